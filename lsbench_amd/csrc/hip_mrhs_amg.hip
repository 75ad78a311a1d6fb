// Several right-hand sides under AMG: the V-cycle of hip_amg.hip on interleaved blocks of KP = 2, 4 or 8
// columns, and the PCG sweeps of hip_mrhs.hip with z as a block of its own (drivers: amg_cycle in
// hip_amg_drv.c, hip_mrhs_drv.c).  An iteration is SpMM, k_amg_mrhs_update_xr, the cycle, k_amg_mrhs_update_p.
//
// Layout: hip_mrhs.hip's -- element (i, c) at i KP + c, 16-byte aligned -- on every level of the hierarchy.
// Every matrix of the hierarchy (A, P, R of a level, the dense coarse inverse) is streamed once for all KP
// columns; a gather of row `col` is KP contiguous doubles.
//
// Rounding rule: each column's arithmetic is hip_amg.hip's amg_row<L> / amg_finish<MODE> exactly -- lane l of a
// row's L takes entries offs[i] + l, + L, ... in storage order through the chain a = fma(val, x, a), the L sums
// are folded by the xor butterfly L/2, ..., 1, and lane 0 applies the same finishing expression.  With the
// level's own `lanes` a column of the block therefore has the BITS of the single-column cycle, whatever the
// other columns hold; columns never mix, so a NaN stays in its column.
//
// Records: the SWEEP form with REC leaves, per workgroup, one record of 2 KP doubles -- b_c . y_c per column,
// then b_c . b_c per column -- in the format k_mrhs_update_p reads (wg_sum_records<2 KP>: fixed order, no
// atomics).  On the fine level's last sweep b is the residual block and y is z, so (r.z, r.r) of every column
// come out of the launch that writes z and the iteration has no dot-product launch.  A one-level hierarchy
// has no sweep: k_amg_dot2_m forms the records behind the dense solve.
//
// Gating: every kernel of the cycle takes a const lsb_mrhs_state * and is a no-op once running == 0 (NULL:
// always run); none writes the state, so the word is never set and tested in the same launch.  Frozen columns
// are computed along with the rest and nobody reads them.  The sweeps gate per column on the status words as
// hip_mrhs.hip's do: a frozen column's stores are skipped, nothing is multiplied by zero.
#include "hip_kcommon.h"
#include "hip_mrhs_k.h"

// --------------------------------------------------------------------------
// One matrix of the hierarchy times a block, L lanes per row, rows dealt to the workgroups in contiguous,
// XCD-contiguous ranges as k_spmm_csr deals them (which rows a workgroup takes does not enter a row's bits).
//   SWEEP  y = xin + minv (b - A xin), out of place      RESID  y = b - A xin
//   SPMV   y = M xin, M rectangular (the restriction)    ADDP   y += P xin, in place (row i reads y_i only)
// --------------------------------------------------------------------------
template <int L, int KP, int MODE, bool REC>
__global__ __launch_bounds__(WG) void k_amg_csr_m(unsigned n, unsigned rows_per_wg, const int *__restrict__ offs,
                                                  const int *__restrict__ cols, const double *__restrict__ vals,
                                                  const double *xin, const double *b, const double *minv, double *y,
                                                  double *__restrict__ records, const lsb_mrhs_state *st) {
  static_assert(!REC || MODE == LSB_AMG_SWEEP, "only a sweep leaves records");
  constexpr int H = KP / 2;
  constexpr unsigned SLOTS = WG / L;
  constexpr int ND = REC ? 2 * KP : 1;
  if (st && !st->running)
    return;
  const unsigned tid = threadIdx.x, slot = tid / L, l = tid % L;
  const unsigned w = xcd_contiguous_wg();
  const unsigned ra = min(w * rows_per_wg, n), rb = min(ra + rows_per_wg, n);
  const d2v *x2 = (const d2v *)xin, *b2 = (const d2v *)b;
  d2v *y2 = (d2v *)y;
  double dot[ND];
#pragma unroll
  for (int k = 0; k < ND; k++)
    dot[k] = 0.0;
  for (unsigned base = ra; base < rb; base += SLOTS) {
    const unsigned r = base + slot;
    double a[KP];
#pragma unroll
    for (int k = 0; k < KP; k++)
      a[k] = 0.0;
    if (r < rb) {
      const int j1 = offs[r + 1];
      for (int j = offs[r] + (int)l; j < j1; j += L) {
        const double v = vals[j];
        const size_t c = (size_t)cols[j] * H;
#pragma unroll
        for (int h = 0; h < H; h++) {
          const d2v t = x2[c + h];
          a[2 * h] = fma(v, t.x, a[2 * h]);
          a[2 * h + 1] = fma(v, t.y, a[2 * h + 1]);
        }
      }
    }
#pragma unroll
    for (int off = L >> 1; off > 0; off >>= 1) {
#pragma unroll
      for (int k = 0; k < KP; k++)
        a[k] += __shfl_xor(a[k], off, 64);
    }
    if (r < rb && l == 0) {
      const size_t o = (size_t)r * H;
#pragma unroll
      for (int h = 0; h < H; h++) {
        d2v s = {a[2 * h], a[2 * h + 1]};
        if constexpr (MODE == LSB_AMG_SWEEP) {
          const d2v bv = b2[o + h], xv = x2[o + h];
          const double m = minv[r];
          s.x = fma(m, bv.x - s.x, xv.x);
          s.y = fma(m, bv.y - s.y, xv.y);
          if constexpr (REC) {
            dot[2 * h] = fma(bv.x, s.x, dot[2 * h]);
            dot[2 * h + 1] = fma(bv.y, s.y, dot[2 * h + 1]);
            dot[KP + 2 * h] = fma(bv.x, bv.x, dot[KP + 2 * h]);
            dot[KP + 2 * h + 1] = fma(bv.y, bv.y, dot[KP + 2 * h + 1]);
          }
        } else if constexpr (MODE == LSB_AMG_RESID) {
          const d2v bv = b2[o + h];
          s.x = bv.x - s.x;
          s.y = bv.y - s.y;
        } else if constexpr (MODE == LSB_AMG_ADDP) {
          const d2v yv = y2[o + h];
          s.x = yv.x + s.x;
          s.y = yv.y + s.y;
        }
        y2[o + h] = s;
      }
    }
  }
  if constexpr (REC) {
    __shared__ double sred[4 * ND];
    wg_sum<ND>(dot, sred);
    if (tid == 0) {
#pragma unroll
      for (int k = 0; k < ND; k++)
        records[(size_t)w * ND + k] = dot[k];
    }
  }
}

// X = minv .* B: a stream at 16 B per lane
template <int KP>
__global__ __launch_bounds__(WG) void k_amg_first_m(unsigned n, const double *__restrict__ b,
                                                    const double *__restrict__ minv, double *__restrict__ x,
                                                    const lsb_mrhs_state *st) {
  constexpr int H = KP / 2;
  if (st && !st->running)
    return;
  const size_t npair = (size_t)n * H, gsz = (size_t)gridDim.x * WG;
  const d2v *b2 = (const d2v *)b;
  d2v *x2 = (d2v *)x;
  for (size_t j = (size_t)blockIdx.x * WG + threadIdx.x; j < npair; j += gsz) {
    const d2v bv = b2[j];
    const double m = minv[j / H];
    d2v xv;
    xv.x = m * bv.x, xv.y = m * bv.y;
    x2[j] = xv;
  }
}

// the dense nc x nc coarse inverse times a block: amg_dense_row<L>'s order per column
template <int L, int KP>
__global__ __launch_bounds__(WG) void k_amg_dense_m(unsigned nc, const double *__restrict__ c,
                                                    const double *__restrict__ b, double *__restrict__ out,
                                                    const lsb_mrhs_state *st) {
  constexpr int H = KP / 2;
  constexpr unsigned SLOTS = WG / L;
  if (st && !st->running)
    return;
  const unsigned slot = threadIdx.x / L, l = threadIdx.x % L;
  const d2v *b2 = (const d2v *)b;
  d2v *o2 = (d2v *)out;
  for (unsigned base = blockIdx.x * SLOTS; base < nc; base += gridDim.x * SLOTS) {
    const unsigned i = base + slot;
    double a[KP];
#pragma unroll
    for (int k = 0; k < KP; k++)
      a[k] = 0.0;
    if (i < nc) {
      const double *ci = c + (size_t)i * nc;
      for (unsigned j = l; j < nc; j += L) {
        const double v = ci[j];
#pragma unroll
        for (int h = 0; h < H; h++) {
          const d2v t = b2[(size_t)j * H + h];
          a[2 * h] = fma(v, t.x, a[2 * h]);
          a[2 * h + 1] = fma(v, t.y, a[2 * h + 1]);
        }
      }
    }
#pragma unroll
    for (int off = L >> 1; off > 0; off >>= 1) {
#pragma unroll
      for (int k = 0; k < KP; k++)
        a[k] += __shfl_xor(a[k], off, 64);
    }
    if (i < nc && l == 0) {
#pragma unroll
      for (int h = 0; h < H; h++)
        o2[(size_t)i * H + h] = d2v{a[2 * h], a[2 * h + 1]};
    }
  }
}

// one record (r.z per column, then r.r per column) per workgroup: the records of a one-level hierarchy
template <int KP>
__global__ __launch_bounds__(WG) void k_amg_dot2_m(unsigned n, const double *__restrict__ r,
                                                   const double *__restrict__ z, double *__restrict__ records,
                                                   const lsb_mrhs_state *st) {
  constexpr int H = KP / 2;
  __shared__ double sred[8 * KP], sout[2 * KP];
  if (st && !st->running)
    return;
  const size_t npair = (size_t)n * H, gsz = (size_t)gridDim.x * WG;
  const d2v *r2 = (const d2v *)r, *z2 = (const d2v *)z;
  double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
  for (size_t j = (size_t)blockIdx.x * WG + threadIdx.x; j < npair; j += gsz) {
    const d2v rv = r2[j], zv = z2[j];
    acc[0][0] += rv.x * zv.x, acc[0][1] += rv.y * zv.y;
    acc[1][0] += rv.x * rv.x, acc[1][1] += rv.y * rv.y;
  }
  wg_sum_cols<KP, 2>(acc, sred, sout);
  if (threadIdx.x < 2 * KP)
    records[(size_t)blockIdx.x * 2 * KP + threadIdx.x] = sout[threadIdx.x];
}

// --------------------------------------------------------------------------
// The PCG sweeps around the cycle.  Bookkeeping as in hip_mrhs.hip: written by workgroup 0, the same decision
// in every workgroup from the same records.
// --------------------------------------------------------------------------
// x = 0, r = b (the cycle on r follows, then k_amg_mrhs_init_p)
template <int KP>
__global__ __launch_bounds__(WG) void k_amg_mrhs_init(unsigned n, const double *__restrict__ b,
                                                      double *__restrict__ x, double *__restrict__ r) {
  const size_t npair = (size_t)n * (KP / 2), gsz = (size_t)gridDim.x * WG;
  const d2v *b2 = (const d2v *)b;
  d2v *x2 = (d2v *)x, *r2 = (d2v *)r;
  for (size_t j = (size_t)blockIdx.x * WG + threadIdx.x; j < npair; j += gsz) {
    x2[j] = d2v{0.0, 0.0};
    r2[j] = b2[j];
  }
}

// p = z ; one record (b.z per column, then b.b per column) per workgroup, for k_mrhs_init_state
template <int KP>
__global__ __launch_bounds__(WG) void k_amg_mrhs_init_p(unsigned n, const double *__restrict__ b,
                                                        const double *__restrict__ z, double *__restrict__ p,
                                                        double *__restrict__ partials2) {
  __shared__ double sred[8 * KP], sout[2 * KP];
  const size_t npair = (size_t)n * (KP / 2), gsz = (size_t)gridDim.x * WG;
  const d2v *b2 = (const d2v *)b, *z2 = (const d2v *)z;
  d2v *p2 = (d2v *)p;
  double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
  for (size_t j = (size_t)blockIdx.x * WG + threadIdx.x; j < npair; j += gsz) {
    const d2v bv = b2[j], zv = z2[j];
    p2[j] = zv;
    acc[0][0] += bv.x * zv.x, acc[0][1] += bv.y * zv.y;
    acc[1][0] += bv.x * bv.x, acc[1][1] += bv.y * bv.y;
  }
  wg_sum_cols<KP, 2>(acc, sred, sout);
  if (threadIdx.x < 2 * KP)
    partials2[(size_t)blockIdx.x * 2 * KP + threadIdx.x] = sout[threadIdx.x];
}

// alpha_c = rz_c / pq_c ; x_c += alpha_c p_c ; r_c -= alpha_c q_c.  k_mrhs_update_xr's alpha, breakdown and
// nspmm bookkeeping; no dot products of its own: (r.z, r.r) come out of the cycle behind it.
template <int KP>
__global__ __launch_bounds__(WG, 8) void k_amg_mrhs_update_xr(unsigned n, const double *__restrict__ p,
                                                           const double *__restrict__ q, double *__restrict__ x,
                                                           double *__restrict__ r, lsb_mrhs_state *__restrict__ st,
                                                           int parity, const double *__restrict__ pq_parts,
                                                           unsigned npq) {
  constexpr int H = KP / 2;
  __shared__ double sred[4 * KP], spq[KP], salpha[KP];
  __shared__ int sact[KP], sent[KP];
  const unsigned tid = threadIdx.x;
  const size_t gtid = (size_t)blockIdx.x * WG + tid, gsz = (size_t)gridDim.x * WG;
  const size_t npair = (size_t)n * H;
  const d2v *p2 = (const d2v *)p, *q2 = (const d2v *)q;
  d2v *x2 = (d2v *)x, *r2 = (d2v *)r;
  d2v pv = {0.0, 0.0}, qv = pv, xv = pv, rv = pv;
  const bool first = gtid < npair;
  if (first)
    pv = p2[gtid], qv = q2[gtid], xv = x2[gtid], rv = r2[gtid];
  wg_sum_records<KP>(pq_parts, npq, sred, spq);
  if (tid < KP) {
    lsb_pcg_state *c = &st->c[tid];
    const int entered = c->status == LSB_STATUS_RUNNING;
    int act = 0;
    double alpha = 0.0;
    if (entered) {
      const double pq = spq[tid];
      if (!(pq != 0.0) || !isfinite(pq)) { // the same decision in every workgroup
        if (blockIdx.x == 0)
          c->status = LSB_STATUS_BREAKDOWN;
      } else {
        alpha = c->rz[parity] / pq;
        act = 1;
        if (blockIdx.x == 0)
          c->pq = pq;
      }
    }
    sent[tid] = entered, sact[tid] = act, salpha[tid] = alpha;
  }
  __syncthreads();
  int any = 0, anyent = 0;
#pragma unroll
  for (int k = 0; k < KP; k++)
    any |= sact[k], anyent |= sent[k];
  if (blockIdx.x == 0 && tid == 0 && anyent) {
    st->nspmm += 1; // the SpMM in front of this launch worked
    if (!any)
      st->running = 0; // the last columns broke down: the cycle behind this launch is a no-op
  }
  if (!any)
    return;
  const unsigned c0 = (2u * tid) % KP;
  const int a0 = sact[c0], a1 = sact[c0 + 1];
  const double al0 = salpha[c0], al1 = salpha[c0 + 1];
  if (first && (a0 | a1)) {
    size_t j = gtid;
    for (;;) {
      xv.x += al0 * pv.x, xv.y += al1 * pv.y;
      rv.x -= al0 * qv.x, rv.y -= al1 * qv.y;
      if (a0 & a1) {
        x2[j] = xv, r2[j] = rv;
      } else if (a0) { // the other column is frozen: its half is not stored
        x[2 * j] = xv.x, r[2 * j] = rv.x;
      } else {
        x[2 * j + 1] = xv.y, r[2 * j + 1] = rv.y;
      }
      j += gsz;
      if (j >= npair)
        break;
      pv = p2[j], qv = q2[j], xv = x2[j], rv = r2[j];
    }
  }
}

// (rz'_c, rr_c) = sum of the cycle's records ; stop test ; beta_c = rz'_c / rz_c ; p_c = z_c + beta_c p_c
template <int KP>
__global__ __launch_bounds__(WG, 8) void k_amg_mrhs_update_p(unsigned n, const double *__restrict__ z,
                                                          double *__restrict__ p, lsb_mrhs_state *__restrict__ st,
                                                          int parity, const double *__restrict__ parts2,
                                                          unsigned nparts2) {
  constexpr int H = KP / 2;
  __shared__ double sred[8 * KP], s2[2 * KP], sbeta[KP];
  __shared__ int sact[KP], sent[KP], sleft[KP];
  const unsigned tid = threadIdx.x;
  const size_t gtid = (size_t)blockIdx.x * WG + tid, gsz = (size_t)gridDim.x * WG;
  const size_t npair = (size_t)n * H;
  const d2v *z2 = (const d2v *)z;
  d2v *p2 = (d2v *)p;
  d2v zv = {0.0, 0.0}, pv = zv;
  const bool first = gtid < npair;
  if (first)
    zv = z2[gtid], pv = p2[gtid];
  wg_sum_records<2 * KP>(parts2, nparts2, sred, s2);
  if (tid < KP) {
    lsb_pcg_state *c = &st->c[tid];
    const int entered = c->status == LSB_STATUS_RUNNING;
    int act = 0, left = 0;
    double beta = 0.0;
    if (entered) {
      const double rz_new = s2[tid], rr = s2[KP + tid];
      const bool conv = rr <= c->thresh2;
      left = !conv;
      if (blockIdx.x == 0) { // only this thread touches the column's iters / rr / rz[parity ^ 1] / status
        const int it = c->iters + 1;
        c->iters = it;
        c->rr = rr;
        c->rz[parity ^ 1] = rz_new;
        if (conv)
          c->status = LSB_STATUS_CONVERGED;
        else if (it >= c->maxit)
          c->status = LSB_STATUS_MAXIT, left = 0;
      }
      if (!conv) {
        beta = rz_new / c->rz[parity];
        act = 1;
      }
    }
    sent[tid] = entered, sact[tid] = act, sbeta[tid] = beta, sleft[tid] = left;
  }
  __syncthreads();
  int any = 0, anyent = 0, anyleft = 0;
#pragma unroll
  for (int k = 0; k < KP; k++)
    any |= sact[k], anyent |= sent[k], anyleft |= sleft[k];
  if (blockIdx.x == 0 && tid == 0 && anyent && !anyleft)
    st->running = 0; // this launch saw the last column stop
  if (!any)
    return;
  const unsigned c0 = (2u * tid) % KP;
  const int a0 = sact[c0], a1 = sact[c0 + 1];
  const double be0 = sbeta[c0], be1 = sbeta[c0 + 1];
  if (first && (a0 | a1)) {
    size_t j = gtid;
    for (;;) {
      pv.x = pnew_of(1.0, zv.x, be0, pv.x); // one expression for every kernel that forms p
      pv.y = pnew_of(1.0, zv.y, be1, pv.y);
      if (a0 & a1)
        p2[j] = pv;
      else if (a0)
        p[2 * j] = pv.x;
      else
        p[2 * j + 1] = pv.y;
      j += gsz;
      if (j >= npair)
        break;
      zv = z2[j], pv = p2[j];
    }
  }
}

// --------------------------------------------------------------------------
// opts.verify, the in-place restart (hip_mrhs.hip) around a cycle: q = b - S x and the records of q_c . q_c
// come from k_spmm_csr's residual form; k_amg_mrhs_restart_r stores r = q for the restarting columns, the
// cycle (not gated: no column is running) forms z of every column, k_amg_mrhs_restart_p stores p = z for the
// restarting columns and leaves one record (r.z per column) for k_mrhs_restart_state.  Both take
// k_mrhs_restart's decision from the same state and records; the cycle between them writes neither.
// --------------------------------------------------------------------------
template <int KP>
__device__ __forceinline__ void restart_decision(const lsb_mrhs_state *st, const double *rr_parts, unsigned nrr,
                                                 int more, double *sred, double *srr, int *sact) {
  wg_sum_records<KP>(rr_parts, nrr, sred, srr);
  if (threadIdx.x < KP) {
    const lsb_pcg_state *c = &st->c[threadIdx.x];
    sact[threadIdx.x] = more && c->iters < c->maxit && mrhs_misses(c, srr[threadIdx.x], st->tol);
  }
  __syncthreads();
}

template <int KP>
__global__ __launch_bounds__(WG) void k_amg_mrhs_restart_r(unsigned n, const double *__restrict__ q,
                                                           double *__restrict__ r,
                                                           const lsb_mrhs_state *__restrict__ st,
                                                           const double *__restrict__ rr_parts, unsigned nrr,
                                                           int more) {
  __shared__ double sred[4 * KP], srr[KP];
  __shared__ int sact[KP];
  const size_t npair = (size_t)n * (KP / 2), gsz = (size_t)gridDim.x * WG;
  const d2v *q2 = (const d2v *)q;
  d2v *r2 = (d2v *)r;
  restart_decision<KP>(st, rr_parts, nrr, more, sred, srr, sact);
  const unsigned c0 = (2u * threadIdx.x) % KP;
  const int a0 = sact[c0], a1 = sact[c0 + 1];
  if (!(a0 | a1))
    return;
  for (size_t j = (size_t)blockIdx.x * WG + threadIdx.x; j < npair; j += gsz) {
    const d2v rv = q2[j];
    if (a0 & a1)
      r2[j] = rv;
    else if (a0)
      r[2 * j] = rv.x;
    else
      r[2 * j + 1] = rv.y;
  }
}

template <int KP>
__global__ __launch_bounds__(WG) void k_amg_mrhs_restart_p(unsigned n, const double *__restrict__ r,
                                                           const double *__restrict__ z, double *__restrict__ p,
                                                           const lsb_mrhs_state *__restrict__ st,
                                                           const double *__restrict__ rr_parts, unsigned nrr,
                                                           int more, double *__restrict__ partials) {
  __shared__ double sred[4 * KP], srr[KP], sout[KP];
  __shared__ int sact[KP];
  const size_t npair = (size_t)n * (KP / 2), gsz = (size_t)gridDim.x * WG;
  const d2v *r2 = (const d2v *)r, *z2 = (const d2v *)z;
  d2v *p2 = (d2v *)p;
  restart_decision<KP>(st, rr_parts, nrr, more, sred, srr, sact);
  const unsigned c0 = (2u * threadIdx.x) % KP;
  const int a0 = sact[c0], a1 = sact[c0 + 1];
  double acc[1][2] = {{0.0, 0.0}};
  if (a0 | a1) {
    for (size_t j = (size_t)blockIdx.x * WG + threadIdx.x; j < npair; j += gsz) {
      const d2v rv = r2[j], zv = z2[j];
      if (a0 & a1)
        p2[j] = zv;
      else if (a0)
        p[2 * j] = zv.x;
      else
        p[2 * j + 1] = zv.y;
      acc[0][0] += rv.x * zv.x, acc[0][1] += rv.y * zv.y;
    }
  }
  wg_sum_cols<KP, 1>(acc, sred, sout);
  if (threadIdx.x < KP)
    partials[(size_t)blockIdx.x * KP + threadIdx.x] = sout[threadIdx.x];
}

// --------------------------------------------------------------------------
// Launchers (C ABI).  kp: 2, 4 or 8.
// --------------------------------------------------------------------------
template <int KP, int MODE, bool REC>
static void amg_csr_launch(const struct lsb_amg_mat *m, unsigned g, const double *xin, const double *b,
                           const double *minv, double *y, double *records, const struct lsb_mrhs_state *st,
                           hipStream_t s) {
  L_DISPATCH(m->lanes, (k_amg_csr_m<L, KP, MODE, REC><<<g, WG, 0, s>>>(m->rows, round_up(div_up(m->rows, g), WG / L),
                                                                       m->offs, m->cols, m->vals, xin, b, minv, y,
                                                                       records, st)));
}

extern "C" {

void lsb_k_amg_first_m(unsigned kp, unsigned n, const double *b, const double *minv, double *x,
                       const struct lsb_mrhs_state *st, void *stream) {
  if (n)
    KP_DISPATCH(kp, (k_amg_first_m<KP><<<sweep_grid(n, kp), WG, 0, (hipStream_t)stream>>>(n, b, minv, x, st)));
}

void lsb_k_amg_csr_m(unsigned kp, int mode, const struct lsb_amg_mat *m, const double *xin, const double *b,
                     const double *minv, double *y, double *records, unsigned *nrecords,
                     const struct lsb_mrhs_state *st, void *stream) {
  if (records && mode != LSB_AMG_SWEEP)
    errx(EXIT_FAILURE, "lsb_k_amg_csr_m: only a sweep leaves records (mode %d)", mode);
  if (!m->rows) {
    if (records)
      errx(EXIT_FAILURE, "lsb_k_amg_csr_m: records of a matrix without rows");
    return;
  }
  hipStream_t s = (hipStream_t)stream;
  const unsigned g = lsb_k_spmm_grid(m->rows, amg_lanes(m->lanes));
  if (nrecords)
    *nrecords = g;
  switch (mode) {
  case LSB_AMG_SWEEP:
    if (records)
      KP_DISPATCH(kp, (amg_csr_launch<KP, LSB_AMG_SWEEP, true>(m, g, xin, b, minv, y, records, st, s)));
    else
      KP_DISPATCH(kp, (amg_csr_launch<KP, LSB_AMG_SWEEP, false>(m, g, xin, b, minv, y, NULL, st, s)));
    break;
  case LSB_AMG_RESID:
    KP_DISPATCH(kp, (amg_csr_launch<KP, LSB_AMG_RESID, false>(m, g, xin, b, minv, y, NULL, st, s)));
    break;
  case LSB_AMG_SPMV:
    KP_DISPATCH(kp, (amg_csr_launch<KP, LSB_AMG_SPMV, false>(m, g, xin, b, minv, y, NULL, st, s)));
    break;
  case LSB_AMG_ADDP:
    KP_DISPATCH(kp, (amg_csr_launch<KP, LSB_AMG_ADDP, false>(m, g, xin, b, minv, y, NULL, st, s)));
    break;
  default:
    errx(EXIT_FAILURE, "lsb_k_amg_csr_m: no mode %d", mode);
  }
}

void lsb_k_amg_dense_m(unsigned kp, unsigned nc, unsigned lanes, const double *cinv, const double *b, double *out,
                       const struct lsb_mrhs_state *st, void *stream) {
  if (!nc)
    return;
  hipStream_t s = (hipStream_t)stream;
  const unsigned Lr = amg_lanes(lanes), g = div_up(nc, WG / Lr);
  KP_DISPATCH(kp, L_DISPATCH(lanes, (k_amg_dense_m<L, KP><<<g, WG, 0, s>>>(nc, cinv, b, out, st))));
}

void lsb_k_amg_dot2_m(unsigned kp, unsigned n, const double *r, const double *z, double *records,
                      unsigned *nrecords, const struct lsb_mrhs_state *st, void *stream) {
  const unsigned g = sweep_grid(n, kp);
  *nrecords = g;
  KP_DISPATCH(kp, (k_amg_dot2_m<KP><<<g, WG, 0, (hipStream_t)stream>>>(n, r, z, records, st)));
}

void lsb_k_amg_mrhs_init(unsigned kp, unsigned n, const double *b, double *x, double *r, void *stream) {
  KP_DISPATCH(kp, (k_amg_mrhs_init<KP><<<sweep_grid(n, kp), WG, 0, (hipStream_t)stream>>>(n, b, x, r)));
}

void lsb_k_amg_mrhs_init_p(unsigned kp, unsigned n, const double *b, const double *z, double *p, double *partials2,
                           unsigned *npartials, void *stream) {
  const unsigned g = sweep_grid(n, kp);
  *npartials = g;
  KP_DISPATCH(kp, (k_amg_mrhs_init_p<KP><<<g, WG, 0, (hipStream_t)stream>>>(n, b, z, p, partials2)));
}

void lsb_k_amg_mrhs_update_xr(unsigned kp, unsigned n, const double *p, const double *q, double *x, double *r,
                              struct lsb_mrhs_state *st, int parity, const double *pq_parts, unsigned npq,
                              void *stream) {
  KP_DISPATCH(kp, (k_amg_mrhs_update_xr<KP><<<sweep_grid(n, kp), WG, 0, (hipStream_t)stream>>>(n, p, q, x, r, st,
                                                                                               parity, pq_parts,
                                                                                               npq)));
}

void lsb_k_amg_mrhs_update_p(unsigned kp, unsigned n, const double *z, double *p, struct lsb_mrhs_state *st,
                             int parity, const double *parts2, unsigned nparts2, void *stream) {
  KP_DISPATCH(kp, (k_amg_mrhs_update_p<KP><<<sweep_grid(n, kp), WG, 0, (hipStream_t)stream>>>(n, z, p, st, parity,
                                                                                              parts2, nparts2)));
}

void lsb_k_amg_mrhs_restart_r(unsigned kp, unsigned n, const double *q, double *r, const struct lsb_mrhs_state *st,
                              const double *rr_parts, unsigned nrr, int more, void *stream) {
  KP_DISPATCH(kp, (k_amg_mrhs_restart_r<KP><<<sweep_grid(n, kp), WG, 0, (hipStream_t)stream>>>(n, q, r, st, rr_parts,
                                                                                               nrr, more)));
}

void lsb_k_amg_mrhs_restart_p(unsigned kp, unsigned n, const double *r, const double *z, double *p,
                              const struct lsb_mrhs_state *st, const double *rr_parts, unsigned nrr, int more,
                              double *partials, unsigned *npartials, void *stream) {
  const unsigned g = sweep_grid(n, kp);
  *npartials = g;
  KP_DISPATCH(kp, (k_amg_mrhs_restart_p<KP><<<g, WG, 0, (hipStream_t)stream>>>(n, r, z, p, st, rr_parts, nrr, more,
                                                                               partials)));
}

} // extern "C"
