// The direct solver's products on blocks of right-hand sides (lsb_hip_solver_solve_direct_multi[_dev],
// _solve_direct_tier_multi[_dev] and their _apply_multi_dev; the host side: direct_tier_enqueue_m in hip_direct_drv.c,
// the work area and the entry points in hip_direct_m_drv.c): the 4 m - 2 launches of hip_direct_t.hip on KP = 2, 4 or 8
// columns at once, every entry of the W_tt, of C and of C^T loaded ONCE per product for all of them.  One tier (the
// single skyline): k_dirt_rows_m<KP, true> and k_dirt_cols_m and nothing else, Z == NULL and not stored.
//
//   round k:  Y_0 = W_00 (P V)_0                      k_dirt_rows_m<KP, true>   V = B in round 1, read through perm
//             t = 1 .. m - 1:
//               Z_t = (P V)_t - C_t Y_<t              k_dirt_fwd_m<KP>
//               Y_t = W_tt Z_t                        k_dirt_rows_m<KP, false>  operand in the tier numbering already
//             Z_(m-1) = W^T Y_(m-1) ; X[perm] (+)= Z  k_dirt_cols_m<KP, FL>
//             t = m - 1 .. 1:
//               Y_j -= sum_i C_t[i, j] Z_i, j < lo_t  k_dirt_bwd_m<KP>          rows of C^T: one owner per row of Y
//               Z_(t-1) = W^T Y_(t-1) ; X[perm] (+)=  k_dirt_cols_m<KP, FL>
//   then k_dir_resid_m and k_dir_step_m of hip_direct_m.hip, as they are.
//
// The rule of the block: a column has the bits of the same column solved alone on the same solver.  Every kernel here
// is its namesake of hip_direct_t.hip per column -- the same lanes per row, the same fma chain in ascending order, the same
// xor butterfly, the same ascending sum of the sixteen partial sums -- and shares only what does not round: the loads
// of vals / cvals / tvals, of first / woff, of the offsets and the column indices.  No MFMA, no atomics, nobody waits
// on another workgroup: the launches are the only ordering.
//
// Block vectors are interleaved as in hip_direct_m.hip: element (i, c) at i KP + c, 16-byte pairs.  B, R and X are in
// the caller's numbering, Y and Z in the tier-major one.  The gate is hip_direct_m.hip's: a launch returns when
// st && !st->running, the round is dirm_round<KP>(st), st == NULL is one un-gated application (V = B, X stored, every
// column written).  Y and Z are work vectors, formed anew in every round, and written for every column; X is gated per
// column, so a frozen column keeps its solution.
#include "hip_mrhs_k.h"

#define DIRT_HIDDEN __attribute__((visibility("hidden")))
#define DIRT_COLS 64
#define DIRT_CWG 1024

typedef unsigned long long dirt_u64;

// Y = W_tt (.) on one tier's workgroups (blk, bwin: the tier's).  PERM: the operand is B or R in the caller's
// numbering, read through perm; else it is Z in the tier-major numbering (passed as b).  A window of at most cap rows
// is staged in LDS (ww KP doubles), a wider one gathered, 8 KP contiguous bytes per entry: the same numbers either way
template <int KP, bool PERM>
__global__ __launch_bounds__(WG) void k_dirt_rows_m(const double *__restrict__ vals, const dirt_u64 *__restrict__ woff,
                                                    const unsigned *__restrict__ first,
                                                    const unsigned *__restrict__ perm, const unsigned *__restrict__ grp,
                                                    const unsigned *__restrict__ blk, const unsigned *__restrict__ bwin,
                                                    unsigned cap, const double *__restrict__ b,
                                                    const double *__restrict__ r, double *__restrict__ t,
                                                    const lsb_mrhs_state *__restrict__ st) {
  constexpr int H = KP / 2;
  extern __shared__ __attribute__((aligned(16))) double win_tm[];
  if (st && !st->running)
    return;
  const d2v *__restrict__ v2 = (const d2v *)(!PERM || !st || dirm_round<KP>(st) == 0 ? b : r);
  d2v *win2 = (d2v *)win_tm;
  const unsigned g0 = blk[blockIdx.x], g1 = blk[blockIdx.x + 1];
  const unsigned wlo = bwin[2 * blockIdx.x], ww = bwin[2 * blockIdx.x + 1];
  const bool staged = ww <= cap;
  if (staged) {
    for (unsigned i = threadIdx.x; i < ww * H; i += WG)
      win2[i] = v2[(size_t)(PERM ? perm[wlo + i / H] : wlo + i / H) * H + i % H];
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
          const d2v *a = v2 + (size_t)(PERM ? perm[f + e] : f + e) * H; // one run of 8 KP bytes per entry
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

// the columns lo .. hi - 1 of one tier: Z_j = (W_tt^T Y)_j, stored for every column of the block where z != NULL, and
// X[perm[j]] = or += Z_j, gated per column.  k_dirt_cols' shape: 64 columns per workgroup from the tier's first row, the window's own
// rows and then the ancestors of its last column inside the tier (parent == n ends the walk), run by run, dealt
// round-robin to the sixteen wavefronts in visiting order; each wavefront adds its rows in ascending k into KP
// accumulators per lane -- ONE load of W for KP fma -- and the sixteen partial sums are added in ascending order.  A
// masked term is fma(0, 0, acc), both factors masked: it leaves acc's bits alone and keeps a NaN of one row or one
// column out of the others, so the number of rows in flight (FL) is free
template <int KP, int FL>
__global__ __launch_bounds__(DIRT_CWG) void k_dirt_cols_m(unsigned n, unsigned lo, unsigned hi,
                                                          const double *__restrict__ vals,
                                                          const dirt_u64 *__restrict__ woff,
                                                          const unsigned *__restrict__ first,
                                                          const unsigned *__restrict__ perm,
                                                          const unsigned *__restrict__ parent,
                                                          const unsigned *__restrict__ run_end,
                                                          const double *__restrict__ t, double *__restrict__ z,
                                                          double *__restrict__ x,
                                                          const lsb_mrhs_state *__restrict__ st) {
  constexpr unsigned NW = DIRT_CWG / 64;
  constexpr int H = KP / 2;
  __shared__ double part[NW][KP][DIRT_COLS];
  if (st && !st->running)
    return;
  const bool add = st && dirm_round<KP>(st) > 0;
  const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const unsigned j0 = lo + blockIdx.x * DIRT_COLS, j1 = (j0 + DIRT_COLS < hi ? j0 + DIRT_COLS : hi) - 1;
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
  for (unsigned p = parent[j1]; p < n;) { // the ancestors of j1 inside the tier, run by run
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
    double s[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
      s[q] = part[0][2 * wave + q][lane];
#pragma unroll
      for (unsigned w = 1; w < NW; w++)
        s[q] += part[w][2 * wave + q][lane];
    }
    if (z) // (uniform over the launch: NULL at one tier, where nobody reads Z)
      ((d2v *)z)[(size_t)j * H + wave] = d2v{s[0], s[1]};
    const int a0 = !st || st->c[2 * wave].status == LSB_STATUS_RUNNING;
    const int a1 = !st || st->c[2 * wave + 1].status == LSB_STATUS_RUNNING;
    if (a0 | a1) {
      const size_t i = (size_t)perm[j] * H + wave;
      double *const xs[1] = {x};
      d2v val[1] = {d2v{s[0], s[1]}};
      if (add) {
        const d2v old = ((const d2v *)x)[i];
        val[0] = d2v{old.x + s[0], old.y + s[1]};
      }
      store_pairs<1>(xs, val, i, a0, a1);
    }
  }
}

// one wavefront per group of rows of a CSR (offs indexed by slot): the row's sums over its entries of vals * V[cols]
// for the KP columns, by dirt_row_sum's lane rule -- lane l takes the entries l, l + L, ... with fma in ascending
// order, the lanes folded by the xor butterfly --, ONE load of vals[e] / cols[e] for KP fma, V's row read as pairs;
// the sums are in the row's lane 0
template <int KP>
__device__ __forceinline__ void dirt_row_sum_m(const unsigned *__restrict__ offs, const unsigned *__restrict__ cols,
                                               const double *__restrict__ vals, const double *__restrict__ v,
                                               unsigned slot, unsigned L, unsigned l, bool mine, unsigned *len,
                                               double (&acc)[KP]) {
  constexpr int H = KP / 2;
#pragma unroll
  for (int c = 0; c < KP; c++)
    acc[c] = 0.0;
  *len = 0;
  if (mine) {
    const unsigned e0 = offs[slot], e1 = offs[slot + 1];
    *len = e1 - e0;
#pragma unroll 2
    for (unsigned e = e0 + l; e < e1; e += L) {
      const double a = vals[e];
      const d2v *__restrict__ vr = (const d2v *)v + (size_t)cols[e] * H;
#pragma unroll
      for (int h = 0; h < H; h++) {
        const d2v p = vr[h];
        acc[2 * h] = fma(a, p.x, acc[2 * h]), acc[2 * h + 1] = fma(a, p.y, acc[2 * h + 1]);
      }
    }
  }
  for (unsigned m = 32; m >= 1; m >>= 1)
    if (m < L) {
#pragma unroll
      for (int c = 0; c < KP; c++)
        acc[c] += __shfl_xor(acc[c], m, 64);
    }
}

// Z_i = (P V)_i - sum_j C[i, j] Y_j for the rows i of one tier (groups g0 .. g1 - 1 of cgrp)
template <int KP>
__global__ __launch_bounds__(WG) void k_dirt_fwd_m(const unsigned *__restrict__ grp, unsigned g0, unsigned g1,
                                                   unsigned lo1, const unsigned *__restrict__ coffs,
                                                   const unsigned *__restrict__ ccols,
                                                   const double *__restrict__ cvals, const unsigned *__restrict__ perm,
                                                   const double *__restrict__ b, const double *__restrict__ r,
                                                   const double *__restrict__ y, double *__restrict__ z,
                                                   const lsb_mrhs_state *__restrict__ st) {
  if (st && !st->running)
    return;
  const double *__restrict__ v = !st || dirm_round<KP>(st) == 0 ? b : r;
  const unsigned g = g0 + blockIdx.x * (WG / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (g >= g1)
    return;
  const unsigned row0 = grp[2 * g], meta = grp[2 * g + 1];
  const unsigned L = meta & 0xffu, nr = meta >> 8, sub = lane / L, l = lane & (L - 1);
  const bool mine = sub < nr;
  const unsigned i = row0 + sub;
  unsigned len;
  double acc[KP];
  dirt_row_sum_m<KP>(coffs, ccols, cvals, y, mine ? i - lo1 : 0u, L, l, mine, &len, acc);
  if (mine && l == 0) {
    double o[KP];
    row_load<KP>(v, perm[i], o);
#pragma unroll
    for (int c = 0; c < KP; c++)
      o[c] = o[c] - acc[c];
    row_store<KP>(z, i, o);
  }
}

// Y_j -= sum_i C[i, j] Z_i over the rows i of one tier, for the rows j below it: the rows of that tier's C^T (toffs:
// the tier's own offsets, indexed by j).  A row the tier does not reach is left as it is
template <int KP>
__global__ __launch_bounds__(WG) void k_dirt_bwd_m(const unsigned *__restrict__ grp, unsigned g0, unsigned g1,
                                                   const unsigned *__restrict__ toffs,
                                                   const unsigned *__restrict__ tcols,
                                                   const double *__restrict__ tvals, const double *__restrict__ z,
                                                   double *__restrict__ y, const lsb_mrhs_state *__restrict__ st) {
  if (st && !st->running)
    return;
  const unsigned g = g0 + blockIdx.x * (WG / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (g >= g1)
    return;
  const unsigned row0 = grp[2 * g], meta = grp[2 * g + 1];
  const unsigned L = meta & 0xffu, nr = meta >> 8, sub = lane / L, l = lane & (L - 1);
  const bool mine = sub < nr;
  const unsigned j = row0 + sub;
  unsigned len;
  double acc[KP];
  dirt_row_sum_m<KP>(toffs, tcols, tvals, z, mine ? j : 0u, L, l, mine, &len, acc);
  if (mine && l == 0 && len) {
    double o[KP];
    row_load<KP>(y, j, o);
#pragma unroll
    for (int c = 0; c < KP; c++)
      o[c] -= acc[c];
    row_store<KP>(y, j, o);
  }
}

// rows in flight per wavefront of k_dirt_cols_m: fewer at the wider blocks, so that nothing spills
template <int KP> struct dirtm_flight { static constexpr int value = KP == 2 ? 8 : 4; };

extern "C" {

// v: Z for the tiers >= 1 (b and r are not read there)
DIRT_HIDDEN void lsb_k_dirt_rows_m(unsigned kp, const struct lsb_dirt_dev *d, unsigned t, const double *b,
                                   const double *r, const double *v, double *y, const struct lsb_mrhs_state *st,
                                   void *stream) {
  const struct lsb_dirt_tier *q = &d->t[t];
  if (!q->nblk)
    return;
  const unsigned rows = q->lds_m[kshift_of(kp) - 1];
  if (t == 0)
    KP_DISPATCH(kp, (k_dirt_rows_m<KP, true><<<q->nblk, WG, (size_t)rows * KP * sizeof(double), (hipStream_t)stream>>>(
                        d->vals, d->woff, d->first, d->perm, d->grp, d->blk + q->blk0, d->bwin + 2 * q->blk0, rows, b,
                        r, y, st)));
  else
    KP_DISPATCH(kp, (k_dirt_rows_m<KP, false><<<q->nblk, WG, (size_t)rows * KP * sizeof(double), (hipStream_t)stream>>>(
                        d->vals, d->woff, d->first, d->perm, d->grp, d->blk + q->blk0, d->bwin + 2 * q->blk0, rows, v,
                        v, y, st)));
}

DIRT_HIDDEN void lsb_k_dirt_cols_m(unsigned kp, const struct lsb_dirt_dev *d, unsigned t, const double *y, double *z,
                                   double *x, const struct lsb_mrhs_state *st, void *stream) {
  const struct lsb_dirt_tier *q = &d->t[t];
  if (q->hi == q->lo)
    return;
  KP_DISPATCH(kp, (k_dirt_cols_m<KP, dirtm_flight<KP>::value>
                   <<<div_up(q->hi - q->lo, DIRT_COLS), DIRT_CWG, 0, (hipStream_t)stream>>>(
                       d->n, q->lo, q->hi, d->vals, d->woff, d->first, d->perm, d->parent, d->run_end, y, z, x, st)));
}

DIRT_HIDDEN void lsb_k_dirt_fwd_m(unsigned kp, const struct lsb_dirt_dev *d, unsigned t, const double *b,
                                  const double *r, const double *y, double *z, const struct lsb_mrhs_state *st,
                                  void *stream) {
  const struct lsb_dirt_tier *q = &d->t[t];
  if (q->cg1 == q->cg0)
    return;
  KP_DISPATCH(kp, (k_dirt_fwd_m<KP><<<div_up(q->cg1 - q->cg0, WG / 64), WG, 0, (hipStream_t)stream>>>(
                      d->cgrp, q->cg0, q->cg1, d->t[1].lo, d->coffs, d->ccols, d->cvals, d->perm, b, r, y, z, st)));
}

DIRT_HIDDEN void lsb_k_dirt_bwd_m(unsigned kp, const struct lsb_dirt_dev *d, unsigned t, const double *z, double *y,
                                  const struct lsb_mrhs_state *st, void *stream) {
  const struct lsb_dirt_tier *q = &d->t[t];
  if (q->tg1 == q->tg0)
    return;
  KP_DISPATCH(kp, (k_dirt_bwd_m<KP><<<div_up(q->tg1 - q->tg0, WG / 64), WG, 0, (hipStream_t)stream>>>(
                      d->tgrp, q->tg0, q->tg1, d->toffs + q->tbase, d->tcols, d->tvals, z, y, st)));
}

} // extern "C"
