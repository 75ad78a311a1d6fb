// The direct solver on blocks of right-hand sides (lsb_hip_solver_solve_direct_multi[_dev], _direct_apply_multi_dev;
// the host side: hip_direct_m_drv.c): the rounds of hip_direct.hip on KP = 2, 4 or 8 columns at once, every entry of W
// loaded ONCE per product for all of them.
//
//   state                                           k_dir_init_state_m (one thread)
//   round k:  T = W (P V)       V = B in round 1     k_dir_rows_m<KP>
//             X (+)= P^T W^T T  stored in round 1    k_dir_cols_m<KP>
//             R = B - S X ; records of r.r, b.b      k_dir_resid_m<L, KP>   (tol = 0: not in the last round)
//             iters = k ; the stop test per column   k_dir_step_m<KP>       (one workgroup)
//
// The rule of every block here: a column of a block has the bits of the same column solved alone.  So each kernel
// keeps the summation order of its single-column twin per column -- the same lanes per row, the same fma chain, the
// same butterfly, the same order of the partial sums -- and only shares what has no rounding: the loads of W, of
// first / woff, of the CSR.  That rules out MFMA (v_mfma_f64_* sums in an order of its own); at <= 8 columns the
// products are nowhere near the fp64 vector rate anyway.
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
#define DIR_COLS 64  // columns per workgroup of k_dir_cols_m: one wavefront's width, as in k_dir_cols
#define DIR_CWG 1024 // ... and its threads: sixteen wavefronts share the rows that reach the window

typedef unsigned long long dir_u64;

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

// T = W (P V).  k_dir_rows' groups, workgroups and windows (the dealing does not depend on the width) and its lane
// rule per column: L lanes per row from the row's length alone, lane l takes entries l, l + L, ... with fma in ascending
// order into KP accumulators from ONE load of w[e], the lanes folded by the xor butterfly.  A window of at most cap
// rows of P V is staged in LDS (ww KP doubles), a wider one gathered from global memory: the same numbers either way
template <int KP>
__global__ __launch_bounds__(WG) void k_dir_rows_m(const double *__restrict__ vals, const dir_u64 *__restrict__ woff,
                                                   const unsigned *__restrict__ first,
                                                   const unsigned *__restrict__ perm, const unsigned *__restrict__ grp,
                                                   const unsigned *__restrict__ blk, const unsigned *__restrict__ bwin,
                                                   unsigned cap, const double *__restrict__ b,
                                                   const double *__restrict__ r, double *__restrict__ t,
                                                   const lsb_mrhs_state *__restrict__ st) {
  constexpr int H = KP / 2;
  extern __shared__ __attribute__((aligned(16))) double win_m[];
  if (st && !st->running)
    return;
  const d2v *__restrict__ v2 = (const d2v *)(!st || dirm_round<KP>(st) == 0 ? b : r);
  d2v *win2 = (d2v *)win_m;
  const unsigned g0 = blk[blockIdx.x], g1 = blk[blockIdx.x + 1];
  const unsigned wlo = bwin[2 * blockIdx.x], ww = bwin[2 * blockIdx.x + 1];
  const bool staged = ww <= cap;
  if (staged) {
    for (unsigned i = threadIdx.x; i < ww * H; i += WG)
      win2[i] = v2[(size_t)perm[wlo + i / H] * H + i % H];
    __syncthreads();
  }
  const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (unsigned g = g0 + wave; g < g1; g += WG / 64) {
    const unsigned row0 = grp[2 * g], meta = grp[2 * g + 1];
    const unsigned L = meta & 0xffu, nr = meta >> 8; // L: a power of two, 1 .. 64; nr <= 64 / L rows
    const unsigned sub = lane / L, l = lane & (L - 1);
    const bool mine = sub < nr;
    double acc[KP];
#pragma unroll
    for (int c = 0; c < KP; c++)
      acc[c] = 0.0;
    if (mine) {
      const unsigned k = row0 + sub, f = first[k], len = k - f + 1;
      const double *__restrict__ w = vals + woff[k];
      if (staged) {
        const d2v *a = win2 + (size_t)(f - wlo) * H;
#pragma unroll 2
        for (unsigned e = l; e < len; e += L) {
          const double we = w[e];
#pragma unroll
          for (int h = 0; h < H; h++) {
            const d2v p = a[(size_t)e * H + h];
            acc[2 * h] = fma(we, p.x, acc[2 * h]), acc[2 * h + 1] = fma(we, p.y, acc[2 * h + 1]);
          }
        }
      } else {
        for (unsigned e = l; e < len; e += L) {
          const double we = w[e];
          const d2v *a = v2 + (size_t)perm[f + e] * H; // one run of 8 KP bytes per entry
#pragma unroll
          for (int h = 0; h < H; h++) {
            const d2v p = a[h];
            acc[2 * h] = fma(we, p.x, acc[2 * h]), acc[2 * h + 1] = fma(we, p.y, acc[2 * h + 1]);
          }
        }
      }
    }
    for (unsigned m = 32; m >= 1; m >>= 1)
      if (m < L) { // (the same L in the whole wavefront)
#pragma unroll
        for (int c = 0; c < KP; c++)
          acc[c] += __shfl_xor(acc[c], m, 64);
      }
    if (mine && l == 0)
      row_store<KP>(t, row0 + sub, acc);
  }
}

// X (+)= P^T W^T T.  k_dir_cols' shape: 64 columns per workgroup, one lane per column in each of sixteen wavefronts,
// the window's own rows and then the ancestors of its last column run by run, dealt round-robin to the wavefronts in
// visiting order; each wavefront adds its own rows in ascending k into KP accumulators per lane -- ONE load of W for
// KP fma -- and the sixteen partial sums are added in ascending order.  Everything about a row (its first column, its
// offset, the KP values of t_k) is wave-uniform and fetched by uniform loads.  A masked term is fma(0, 0, acc), both
// factors masked: it leaves acc's bits alone and keeps a NaN of one row or one column out of the others, so the
// number of rows in flight (FL) is free.  The store is gated per column: a frozen column is not written
template <int KP, int FL>
__global__ __launch_bounds__(DIR_CWG) void k_dir_cols_m(unsigned n, const double *__restrict__ vals,
                                                        const dir_u64 *__restrict__ woff,
                                                        const unsigned *__restrict__ first,
                                                        const unsigned *__restrict__ perm,
                                                        const unsigned *__restrict__ parent,
                                                        const unsigned *__restrict__ run_end,
                                                        const double *__restrict__ t, double *__restrict__ x,
                                                        const lsb_mrhs_state *__restrict__ st) {
  constexpr unsigned NW = DIR_CWG / 64;
  constexpr int H = KP / 2;
  __shared__ double part[NW][KP][DIR_COLS];
  if (st && !st->running)
    return;
  const bool add = st && dirm_round<KP>(st) > 0;
  const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const unsigned j0 = blockIdx.x * DIR_COLS, j1 = (j0 + DIR_COLS < n ? j0 + DIR_COLS : n) - 1;
  const unsigned j = j0 + lane;
  const bool active = j <= j1;
  double acc[KP];
#pragma unroll
  for (int c = 0; c < KP; c++)
    acc[c] = 0.0;
  // this wavefront's rows k0, k0 + NW, ... <= kend, FL at a time: their loads of W are independent of one another
  // and go out together
  auto visit = [&](unsigned k0, unsigned kend) {
    for (unsigned kb = k0; kb <= kend; kb += FL * NW) {
      double w[FL];
      unsigned kk[FL];
      bool in[FL];
#pragma unroll
      for (int u = 0; u < FL; u++) {
        const unsigned k = kb + u * NW;
        kk[u] = k <= kend ? k : kend; // (past the run: its last row again, not added)
        const unsigned f = first[kk[u]];
        in[u] = active && j >= f && j <= kk[u] && k <= kend;
        w[u] = vals[woff[kk[u]] + (in[u] ? j - f : 0u)]; // (every lane loads: no branch between the loads)
      }
#pragma unroll
      for (int u = 0; u < FL; u++) {
        const double *__restrict__ tk = t + (size_t)kk[u] * KP;
        const double wu = in[u] ? w[u] : 0.0;
#pragma unroll
        for (int c = 0; c < KP; c++)
          acc[c] = fma(in[u] ? tk[c] : 0.0, wu, acc[c]);
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
#pragma unroll
  for (int c = 0; c < KP; c++)
    part[wave][c][lane] = acc[c];
  __syncthreads();
  if (wave < (unsigned)H && active) { // wavefront h: the pair of columns 2 h, 2 h + 1
    double z[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
      z[q] = part[0][2 * wave + q][lane];
#pragma unroll
      for (unsigned w = 1; w < NW; w++)
        z[q] += part[w][2 * wave + q][lane];
    }
    const int a0 = !st || st->c[2 * wave].status == LSB_STATUS_RUNNING;
    const int a1 = !st || st->c[2 * wave + 1].status == LSB_STATUS_RUNNING;
    if (a0 | a1) {
      const size_t i = (size_t)perm[j] * H + wave;
      double *const xs[1] = {x};
      d2v val[1] = {d2v{z[0], z[1]}};
      if (add) {
        const d2v old = ((const d2v *)x)[i];
        val[0] = d2v{old.x + z[0], old.y + z[1]};
      }
      store_pairs<1>(xs, val, i, a0, a1);
    }
  }
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

// rows in flight per wavefront of k_dir_cols_m: fewer at the wider blocks, so that nothing spills
template <int KP> struct dirm_flight { static constexpr int value = KP == 2 ? 8 : 4; };

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

// lds_rows: the widest window the launch stages, in rows (<= DIR_LDS_CAP / kp: the host's)
DIR_HIDDEN void lsb_k_dir_rows_m(unsigned kp, const struct lsb_dir_dev *d, unsigned lds_rows, const double *b, const double *r, double *t, const struct lsb_mrhs_state *st,
                                 void *stream) {
  if (!d->nblk)
    return;
  KP_DISPATCH(kp, (k_dir_rows_m<KP><<<d->nblk, WG, (size_t)lds_rows * KP * sizeof(double), (hipStream_t)stream>>>(
                      d->vals, d->woff, d->first, d->perm, d->grp, d->blk, d->bwin, lds_rows, b, r, t, st)));
}

DIR_HIDDEN void lsb_k_dir_cols_m(unsigned kp, const struct lsb_dir_dev *d, const double *t, double *x,
                                 const struct lsb_mrhs_state *st, void *stream) {
  if (!d->n)
    return;
  KP_DISPATCH(kp, (k_dir_cols_m<KP, dirm_flight<KP>::value><<<div_up(d->n, DIR_COLS), DIR_CWG, 0, (hipStream_t)stream>>>(
                      d->n, d->vals, d->woff, d->first, d->perm, d->parent, d->run_end, t, x, st)));
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
