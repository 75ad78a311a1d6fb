// Several right-hand sides at once: the kernels of lsb_hip_solver_solve_multi / _spmm_dev (driver:
// hip_mrhs_drv.c).  KP = 2, 4 or 8 INDEPENDENT PCG recurrences advance through the same launches -- the
// classic form's three per iteration (SpMM, k_mrhs_update_xr, k_mrhs_update_p) -- each column with its own
// alpha, beta, norms, iteration count and status.  This is not block-CG.
//
// Two forms of the preconditioner, ONE set of sweeps (template parameter Z): the diagonal ones, z = dinv .* r
// formed inside the sweeps, and z as a block of its own -- the V-cycle of hip_mrhs_amg.hip runs between
// k_mrhs_update_xr<KP, true> and k_mrhs_update_p<KP, true> and leaves the records the latter reads.  The column
// bookkeeping (alpha and breakdown, stop test and beta, `running`, nspmm, the gated stores, the restart decision
// of a verify round) is the same code in both.
//
// Layout.  The block vectors (b, x, r, p, q) are ROW-MAJOR, INTERLEAVED: element (i, c) at i KP + c,
// 16-byte aligned.  A gather of row `col` is KP contiguous doubles (16 / 32 / 64 B) and every sweep is one
// contiguous stream of n KP doubles.  The sweeps move 16 B per lane; pair j belongs to row j / (KP/2) and to
// columns (2 j mod KP, + 1), and because the grid stride is a multiple of KP a lane keeps its two columns
// over all its trips.
//
// State (lsb_mrhs_state): KP lsb_pcg_state records + one `running` word.  A column whose status != 0 is
// FROZEN: its x, r and p are no longer stored (the stores are skipped, nothing is multiplied by zero: a
// column that broke down may hold NaN); its partial sums are still written and nobody reads them.  The
// sweeps gate per column on the status words and never read `running`; the SpMM gates on `running` alone and
// never writes it: the word is cleared by the sweep that sees the last column stop, so it is never set and
// tested in the same launch.  Bookkeeping is k_pcg_update_p's: the first KP threads of workgroup 0 write,
// every workgroup takes the same decisions from the same partial records, re-reduced in an order that
// depends on their number only (no atomics: the same bits from run to run, and a column's bits do not depend
// on what the other columns hold).
#include "hip_kcommon.h"
#include "hip_mrhs_k.h"

// --------------------------------------------------------------------------
// caller's column-major block (leading dimension ld, caller's numbering) <-> interleaved (internal numbering)
// perm[internal] = caller's row, -1 on a pad row, NULL: the same numbering.  Columns >= nrhs of the
// interleaved block are the batch's padding: zero.
// --------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void k_mrhs_pack(unsigned n, unsigned kshift, unsigned nrhs,
                                                  const int *__restrict__ perm, const double *__restrict__ src,
                                                  size_t ld, double *__restrict__ dst) {
  const size_t total = (size_t)n << kshift;
  for (size_t e = (size_t)blockIdx.x * WG + threadIdx.x; e < total; e += (size_t)gridDim.x * WG) {
    const size_t i = e >> kshift;
    const unsigned c = (unsigned)(e & ((1u << kshift) - 1u));
    const long long j = perm ? (long long)perm[i] : (long long)i;
    dst[e] = (c < nrhs && j >= 0) ? src[(size_t)c * ld + (size_t)j] : 0.0;
  }
}

// writes every column < nrhs, frozen ones included
__global__ __launch_bounds__(WG) void k_mrhs_unpack(unsigned n, unsigned kshift, unsigned nrhs,
                                                    const int *__restrict__ perm, const double *__restrict__ src,
                                                    double *__restrict__ dst, size_t ld) {
  const size_t total = (size_t)n << kshift;
  for (size_t e = (size_t)blockIdx.x * WG + threadIdx.x; e < total; e += (size_t)gridDim.x * WG) {
    const size_t i = e >> kshift;
    const unsigned c = (unsigned)(e & ((1u << kshift) - 1u));
    const long long j = perm ? (long long)perm[i] : (long long)i;
    if (c < nrhs && j >= 0)
      dst[(size_t)c * ld + (size_t)j] = src[e];
  }
}

// --------------------------------------------------------------------------
// Y = S X off a CSR, L lanes per row as k_spmv_subwave<L>: a row's sums are block_row_product's (hip_mrhs_k.h),
// the one rounding rule of DESIGN.md section 4.
// Epilogue, lane 0 of the row: y = S x and the per-column partials of x_c . y_c (the p.q of the iteration).
// One record of KP doubles per workgroup, rows dealt XCD-contiguously.
// st != NULL: a no-op once st->running == 0.
//
// RES: the residual kernel of opts.verify, y = bres - S x and the partials of y_c . y_c.  Where the
// recurrence has converged to 1e-13 the residual is of the size of the ROUNDING of an fp64 S x (config 2,
// column b_i = i: u || |S||x| + |b| || / ||b|| = 7.8e-14 against a residual of 7.7e-14; two fp64 summation
// orders disagree by 3 %), so this form -- one launch per verify round -- carries every product's and every
// addition's rounding error along (two_prod through fma, two_sum; Ogita, Rump & Oishi's Dot2, the butterfly
// folding (sum, error) pairs) and subtracts in the same way: y is b - S x as if formed in twice the working
// precision, then rounded.  The restart starts from that residual.
// --------------------------------------------------------------------------
// (contraction is switched off where the error-free transformations live: a product fused into the
// addition behind it is not the rounded product whose error is carried along)
__device__ __forceinline__ void two_sum(double a, double b, double &s, double &e) {
#pragma clang fp contract(off)
  s = a + b;
  const double bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}

template <int L, int KP, bool RES>
__global__ __launch_bounds__(WG) void k_spmm_csr(unsigned n, unsigned rows_per_wg, const int *__restrict__ offs,
                                                 const int *__restrict__ cols, const double *__restrict__ vals,
                                                 const double *__restrict__ x, double *__restrict__ y,
                                                 const double *__restrict__ bres, double *__restrict__ partials,
                                                 const lsb_mrhs_state *__restrict__ st) {
  constexpr int H = KP / 2;
  constexpr unsigned SLOTS = WG / L;
  constexpr int NE = RES ? KP : 1;
  __shared__ double sred[4 * KP];
  const unsigned tid = threadIdx.x, slot = tid / L, l = tid % L;
  const unsigned w = xcd_contiguous_wg();
  const unsigned ra = min(w * rows_per_wg, n), rb = min(ra + rows_per_wg, n);
  // the word travels with the first row's loads; nothing is stored before it is tested, and no launch
  // that runs beside this one writes it
  const int stopped = st ? !st->running : 0;
  const d2v *x2 = (const d2v *)x, *b2 = (const d2v *)bres;
  d2v *y2 = (d2v *)y;
  double dot[KP];
#pragma unroll
  for (int k = 0; k < KP; k++)
    dot[k] = 0.0;
  for (unsigned base = ra; base < rb; base += SLOTS) {
    const unsigned r = base + slot;
    double a[KP], e[NE]; // e: the rounding errors of a's chain (RES)
#pragma unroll
    for (int k = 0; k < NE; k++)
      e[k] = 0.0;
    if constexpr (!RES) {
      block_row_product<L, KP>(offs, cols, vals, x, r, r < rb, l, a);
    } else {
      // Another computation, not the row rule: the same entries in the same order, but every product and every
      // addition of the loop and of the butterfly carries its rounding error along.  It stays written out here.
#pragma unroll
      for (int k = 0; k < KP; k++)
        a[k] = 0.0;
      if (r < rb) {
        const int j0 = offs[r], j1 = offs[r + 1];
        for (int j = j0 + (int)l; j < j1; j += L) {
          const double v = vals[j];
          const size_t c = (size_t)cols[j] * H;
#pragma unroll
          for (int h = 0; h < H; h++) {
#pragma clang fp contract(off)
            const d2v t = x2[c + h];
            const double tk[2] = {t.x, t.y};
#pragma unroll
            for (int q = 0; q < 2; q++) {
              const double pr = v * tk[q], pe = fma(v, tk[q], -pr);
              double se;
              two_sum(a[2 * h + q], pr, a[2 * h + q], se);
              e[2 * h + q] += pe + se;
            }
          }
        }
      }
#pragma unroll
      for (int off = L >> 1; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < KP; k++) { // both partners form the same sum and the same error
#pragma clang fp contract(off)
          const double ao = __shfl_xor(a[k], off, 64), eo = __shfl_xor(e[k], off, 64);
          double se;
          two_sum(a[k], ao, a[k], se);
          e[k] = (e[k] + eo) + se;
        }
      }
    }
    if (stopped)
      return;
    if (r < rb && l == 0) {
      const size_t o = (size_t)r * H;
#pragma unroll
      for (int h = 0; h < H; h++) {
        d2v s = {a[2 * h], a[2 * h + 1]};
        if constexpr (RES) {
#pragma clang fp contract(off)
          const d2v bv = b2[o + h];
          double t0, t1, te;
          two_sum(bv.x, -s.x, t0, te);
          s.x = t0 + (te - e[2 * h]);
          two_sum(bv.y, -s.y, t1, te);
          s.y = t1 + (te - e[2 * h + 1]);
          dot[2 * h] = fma(s.x, s.x, dot[2 * h]);
          dot[2 * h + 1] = fma(s.y, s.y, dot[2 * h + 1]);
        } else {
          const d2v xd = x2[o + h];
          dot[2 * h] = fma(s.x, xd.x, dot[2 * h]);
          dot[2 * h + 1] = fma(s.y, xd.y, dot[2 * h + 1]);
        }
        y2[o + h] = s;
      }
    }
  }
  if (stopped)
    return;
  wg_sum<KP>(dot, sred);
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < KP; k++)
      partials[(size_t)w * KP + k] = dot[k];
  }
}

// --------------------------------------------------------------------------
// The classic form's three sweeps over interleaved blocks.  dinv == NULL: the constant dc.
// --------------------------------------------------------------------------
// x = 0, r = b, p = dinv.*b ; one record (r.z per column, then b.b per column) per workgroup
template <int KP>
__global__ __launch_bounds__(WG) void k_mrhs_init(unsigned n, const double *__restrict__ b,
                                                  const double *__restrict__ dinv, double dc, double *__restrict__ x,
                                                  double *__restrict__ r, double *__restrict__ p,
                                                  double *__restrict__ partials2) {
  constexpr int H = KP / 2;
  __shared__ double sred[8 * KP], sout[2 * KP];
  const size_t gtid = (size_t)blockIdx.x * WG + threadIdx.x, gsz = (size_t)gridDim.x * WG;
  const size_t npair = (size_t)n * H;
  const d2v *b2 = (const d2v *)b;
  d2v *x2 = (d2v *)x, *r2 = (d2v *)r, *p2 = (d2v *)p;
  double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
  for (size_t j = gtid; j < npair; j += gsz) {
    const d2v bv = b2[j];
    const double d = dinv ? dinv[j / H] : dc;
    d2v pv;
    pv.x = d * bv.x, pv.y = d * bv.y;
    x2[j] = d2v{0.0, 0.0};
    r2[j] = bv;
    p2[j] = pv;
    acc[0][0] += bv.x * pv.x, acc[0][1] += bv.y * pv.y;
    acc[1][0] += bv.x * bv.x, acc[1][1] += bv.y * bv.y;
  }
  wg_sum_cols<KP, 2>(acc, sred, sout);
  if (threadIdx.x < 2 * KP)
    partials2[(size_t)blockIdx.x * 2 * KP + threadIdx.x] = sout[threadIdx.x];
}

// z as a block of its own: x = 0, r = b; the cycle on r follows, then k_amg_dot2_m<KP, true>
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

// one record (u.z per column, then u.u per column) per workgroup over two blocks, in k_mrhs_init's format.
// P: also p = z -- u = b, the records k_mrhs_init_state reads.  Else u = r, the records of an iteration whose
// cycle is a one-level hierarchy and has no sweep to leave them.  st != NULL: a no-op once st->running == 0.
template <int KP, bool P>
__global__ __launch_bounds__(WG) void k_amg_dot2_m(unsigned n, const double *__restrict__ u,
                                                   const double *__restrict__ z, double *__restrict__ p,
                                                   double *__restrict__ records, const lsb_mrhs_state *st) {
  constexpr int H = KP / 2;
  __shared__ double sred[8 * KP], sout[2 * KP];
  if (st && !st->running)
    return;
  const size_t npair = (size_t)n * H, gsz = (size_t)gridDim.x * WG;
  const d2v *u2 = (const d2v *)u, *z2 = (const d2v *)z;
  double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
  for (size_t j = (size_t)blockIdx.x * WG + threadIdx.x; j < npair; j += gsz) {
    const d2v uv = u2[j], zv = z2[j];
    if constexpr (P)
      ((d2v *)p)[j] = zv;
    acc[0][0] += uv.x * zv.x, acc[0][1] += uv.y * zv.y;
    acc[1][0] += uv.x * uv.x, acc[1][1] += uv.y * uv.y;
  }
  wg_sum_cols<KP, 2>(acc, sred, sout);
  if (threadIdx.x < 2 * KP)
    records[(size_t)blockIdx.x * 2 * KP + threadIdx.x] = sout[threadIdx.x];
}

// bb_parts == NULL: a batch from x0 = 0, the records are k_mrhs_init's (r.z, b.b).  Else a batch from an initial
// guess: the records hold (r.z, r.r) of r = b - S x0, b.b comes from k_mrhs_x0_bb's, and a column that starts
// within the tolerance is CONVERGED with 0 iterations, its x untouched.
template <int KP>
__global__ __launch_bounds__(WG) void k_mrhs_init_state(lsb_mrhs_state *__restrict__ st,
                                                        const double *__restrict__ partials2, unsigned nparts,
                                                        const double *__restrict__ bb_parts, unsigned nbb,
                                                        double tol, int maxit) {
  __shared__ double sred[8 * KP], s2[2 * KP], sbb[2 * KP];
  __shared__ int srun[KP];
  wg_sum_records<2 * KP>(partials2, nparts, sred, s2);
  if (bb_parts)
    wg_sum_records<2 * KP>(bb_parts, nbb, sred, sbb);
  const unsigned t = threadIdx.x;
  if (t < KP) {
    lsb_pcg_state *c = &st->c[t];
    const double rz = s2[t], rr = s2[KP + t], bb = bb_parts ? sbb[KP + t] : rr;
    c->rz[0] = rz, c->rz[1] = 0.0;
    c->alpha[0] = c->alpha[1] = 0.0;
    c->bb = bb;
    c->thresh2 = tol * tol * bb;
    c->rr = rr;
    c->pq = 0.0;
    c->iters = 0;
    c->maxit = maxit;
    c->pad = 0, c->xpend = 0, c->pad2_ = 0;
    // b_c == 0 => x_c = 0 is the solution (the padding columns of a batch among them)
    c->status = (bb == 0.0 || (bb_parts && rr <= c->thresh2))
                    ? LSB_STATUS_CONVERGED
                    : (maxit <= 0 ? LSB_STATUS_MAXIT : LSB_STATUS_RUNNING);
    srun[t] = c->status == LSB_STATUS_RUNNING;
    st->true_relres[t] = -1.0;
    st->corrections[t] = 0;
    st->start_relres[t] = bb > 0.0 ? sqrt(rr / bb) : 0.0;
  }
  if (t >= KP && t < LSB_MRHS_MAX) { // the records a narrower batch does not use
    memset(&st->c[t], 0, sizeof st->c[t]);
    st->c[t].status = LSB_STATUS_CONVERGED;
    st->true_relres[t] = -1.0;
    st->corrections[t] = 0;
    st->start_relres[t] = 0.0;
  }
  __syncthreads();
  if (t == 0) {
    int run = 0;
#pragma unroll
    for (int k = 0; k < KP; k++)
      run |= srun[k];
    st->running = run;
    st->nspmm = 0;
    st->tol = tol;
  }
}

// Z == false: the diagonal preconditioners, z = dinv .* r formed on the fly.  Z == true: z is a block of its own,
// written by the launches between the two sweeps (the V-cycle of hip_mrhs_amg.hip, whose last sweep leaves the
// records); dinv, dc and partials2 are not looked at.
//
// alpha_c = rz_c / pq_c ; x_c += alpha_c p_c ; r_c -= alpha_c q_c ; !Z: one record (r.dinv.r per column, then
// r.r per column) per workgroup.  p.q zero or not finite: the column is BREAKDOWN (k_pcg_update_xr's test).
template <int KP, bool Z>
__global__ __launch_bounds__(WG, 8) void k_mrhs_update_xr(unsigned n, const double *__restrict__ p,
                                                       const double *__restrict__ q, const double *__restrict__ dinv,
                                                       double dc, double *__restrict__ x, double *__restrict__ r,
                                                       lsb_mrhs_state *__restrict__ st, int parity,
                                                       const double *__restrict__ pq_parts, unsigned npq,
                                                       double *__restrict__ partials2) {
  constexpr int H = KP / 2;
  __shared__ double sred[(Z ? 4 : 8) * KP], spq[KP], salpha[KP];
  __shared__ int sact[KP], sent[KP];
  const unsigned tid = threadIdx.x;
  const size_t gtid = (size_t)blockIdx.x * WG + tid, gsz = (size_t)gridDim.x * WG;
  const size_t npair = (size_t)n * H;
  const d2v *p2 = (const d2v *)p, *q2 = (const d2v *)q;
  d2v *x2 = (d2v *)x, *r2 = (d2v *)r;
  // as k_pcg_update_xr: the lane's first operands travel with the status words and the partial records
  d2v pv = {0.0, 0.0}, qv = pv, xv = pv, rv = pv;
  double dv = dc;
  const bool first = gtid < npair;
  if (first) {
    pv = p2[gtid], qv = q2[gtid], xv = x2[gtid], rv = r2[gtid];
    if (!Z && dinv)
      dv = dinv[gtid / H];
  }
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
      st->running = 0; // the last columns broke down (Z: the cycle behind this launch is a no-op)
  }
  if (!any)
    return;
  const unsigned c0 = (2u * tid) % KP;
  const int a0 = sact[c0], a1 = sact[c0 + 1];
  const double al0 = salpha[c0], al1 = salpha[c0 + 1];
  double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
  if (first && (a0 | a1)) {
    size_t j = gtid;
    for (;;) {
      xv.x += al0 * pv.x, xv.y += al1 * pv.y;
      rv.x -= al0 * qv.x, rv.y -= al1 * qv.y;
      store_pairs({x, r}, {xv, rv}, j, a0, a1);
      if constexpr (!Z) {
        acc[0][0] += rv.x * (dv * rv.x), acc[0][1] += rv.y * (dv * rv.y);
        acc[1][0] += rv.x * rv.x, acc[1][1] += rv.y * rv.y;
      }
      j += gsz;
      if (j >= npair)
        break;
      pv = p2[j], qv = q2[j], xv = x2[j], rv = r2[j];
      if (!Z && dinv)
        dv = dinv[j / H];
    }
  }
  if constexpr (!Z) {
    __shared__ double sout[2 * KP];
    wg_sum_cols<KP, 2>(acc, sred, sout);
    if (tid < 2 * KP)
      partials2[(size_t)blockIdx.x * 2 * KP + tid] = sout[tid];
  }
}

// (rz'_c, rr_c) = sum of the records ; stop test ; beta_c = rz'_c / rz_c ; p_c = z_c + beta_c p_c, z_c = dinv .* r_c
// or -- Z -- column c of the block zr
template <int KP, bool Z>
__global__ __launch_bounds__(WG, Z ? 8 : 0) void k_mrhs_update_p(unsigned n, const double *__restrict__ zr,
                                                                 const double *__restrict__ dinv, double dc,
                                                                 double *__restrict__ p,
                                                                 lsb_mrhs_state *__restrict__ st, int parity,
                                                                 const double *__restrict__ parts2,
                                                                 unsigned nparts2) {
  constexpr int H = KP / 2;
  __shared__ double sred[8 * KP], s2[2 * KP], sbeta[KP];
  __shared__ int sact[KP], sent[KP], sleft[KP];
  const unsigned tid = threadIdx.x;
  const size_t gtid = (size_t)blockIdx.x * WG + tid, gsz = (size_t)gridDim.x * WG;
  const size_t npair = (size_t)n * H;
  const d2v *zr2 = (const d2v *)zr;
  d2v *p2 = (d2v *)p;
  d2v rv = {0.0, 0.0}, pv = rv;
  double dv = dc;
  const bool first = gtid < npair;
  if (first) {
    rv = zr2[gtid], pv = p2[gtid];
    if (!Z && dinv)
      dv = dinv[gtid / H];
  }
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
      if constexpr (Z) { // one expression for every kernel that forms p; the literal folds d * r
        pv.x = pnew_of(1.0, rv.x, be0, pv.x);
        pv.y = pnew_of(1.0, rv.y, be1, pv.y);
      } else {
        pv.x = pnew_of(dv, rv.x, be0, pv.x);
        pv.y = pnew_of(dv, rv.y, be1, pv.y);
      }
      store_pairs({p}, {pv}, j, a0, a1);
      j += gsz;
      if (j >= npair)
        break;
      rv = zr2[j], pv = p2[j];
      if (!Z && dinv)
        dv = dinv[j / H];
    }
  }
}

// --------------------------------------------------------------------------
// opts.verify: the in-place restart of the columns the recurrence called converged but whose residual
// RECOMPUTED from x (q = b - S x and the records of q_c . q_c, from k_spmm_csr's epilogue) misses the
// tolerance: r = q, p = D^-1 r, x kept, bb and the threshold unchanged, iterations counted on.  Every other
// column stays frozen.  more == 0: no round is left, such a column becomes MAXIT.
// --------------------------------------------------------------------------
// the sweep: reads the state, writes r and p of the restarting columns and one record (r.dinv.r per column)
template <int KP>
__global__ __launch_bounds__(WG) void k_mrhs_restart(unsigned n, const double *__restrict__ q,
                                                     const double *__restrict__ dinv, double dc,
                                                     double *__restrict__ r, double *__restrict__ p,
                                                     const lsb_mrhs_state *__restrict__ st,
                                                     const double *__restrict__ rr_parts, unsigned nrr, int more,
                                                     double *__restrict__ partials) {
  constexpr int H = KP / 2;
  __shared__ double sred[4 * KP], srr[KP], sout[KP];
  __shared__ int sact[KP];
  const unsigned tid = threadIdx.x;
  const size_t gtid = (size_t)blockIdx.x * WG + tid, gsz = (size_t)gridDim.x * WG;
  const size_t npair = (size_t)n * H;
  const d2v *q2 = (const d2v *)q;
  restart_decision<KP>(st, rr_parts, nrr, more, sred, srr, sact);
  const unsigned c0 = (2u * tid) % KP;
  const int a0 = sact[c0], a1 = sact[c0 + 1];
  double acc[1][2] = {{0.0, 0.0}};
  if (a0 | a1) {
    for (size_t j = gtid; j < npair; j += gsz) {
      const d2v rv = q2[j];
      const double dv = dinv ? dinv[j / H] : dc;
      d2v pv;
      pv.x = dv * rv.x, pv.y = dv * rv.y;
      store_pairs({r, p}, {rv, pv}, j, a0, a1);
      acc[0][0] += rv.x * pv.x, acc[0][1] += rv.y * pv.y;
    }
  }
  wg_sum_cols<KP, 1>(acc, sred, sout);
  if (tid < KP)
    partials[(size_t)blockIdx.x * KP + tid] = sout[tid];
}

// The same round with z as a block of its own: k_amg_mrhs_restart_r stores r = q for the restarting columns, the
// cycle (not gated: no column is running) forms z of every column, k_amg_mrhs_restart_p stores p = z for the
// restarting columns and leaves one record (r.z per column).  Both take k_mrhs_restart's decision from the same
// state and records; the cycle between them writes neither.
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
  restart_decision<KP>(st, rr_parts, nrr, more, sred, srr, sact);
  const unsigned c0 = (2u * threadIdx.x) % KP;
  const int a0 = sact[c0], a1 = sact[c0 + 1];
  if (!(a0 | a1))
    return;
  for (size_t j = (size_t)blockIdx.x * WG + threadIdx.x; j < npair; j += gsz)
    store_pairs({r}, {q2[j]}, j, a0, a1);
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
  restart_decision<KP>(st, rr_parts, nrr, more, sred, srr, sact);
  const unsigned c0 = (2u * threadIdx.x) % KP;
  const int a0 = sact[c0], a1 = sact[c0 + 1];
  double acc[1][2] = {{0.0, 0.0}};
  if (a0 | a1) {
    for (size_t j = (size_t)blockIdx.x * WG + threadIdx.x; j < npair; j += gsz) {
      const d2v rv = r2[j], zv = z2[j];
      store_pairs({p}, {zv}, j, a0, a1);
      acc[0][0] += rv.x * zv.x, acc[0][1] += rv.y * zv.y;
    }
  }
  wg_sum_cols<KP, 1>(acc, sred, sout);
  if (threadIdx.x < KP)
    partials[(size_t)blockIdx.x * KP + threadIdx.x] = sout[threadIdx.x];
}

// one workgroup, behind the sweep: the same decisions, written down
template <int KP>
__global__ __launch_bounds__(WG) void k_mrhs_restart_state(lsb_mrhs_state *__restrict__ st,
                                                           const double *__restrict__ rr_parts, unsigned nrr,
                                                           const double *__restrict__ rz_parts, unsigned nrz,
                                                           int more) {
  __shared__ double sred[4 * KP], srr[KP], srz[KP];
  __shared__ int srun[KP];
  wg_sum_records<KP>(rr_parts, nrr, sred, srr);
  wg_sum_records<KP>(rz_parts, nrz, sred, srz);
  const unsigned t = threadIdx.x;
  if (t < KP) {
    lsb_pcg_state *c = &st->c[t];
    const double rr = srr[t];
    if (c->bb > 0.0)
      st->true_relres[t] = mrhs_true_relres(c, rr);
    if (mrhs_misses(c, rr, st->tol)) {
      if (more && c->iters < c->maxit) {
        c->rz[0] = srz[t], c->rz[1] = 0.0;
        c->rr = rr;
        c->status = LSB_STATUS_RUNNING;
        st->corrections[t] += 1;
      } else {
        c->rr = rr;
        c->status = LSB_STATUS_MAXIT; // the corrections did not get there: not converged
      }
    }
    srun[t] = c->status == LSB_STATUS_RUNNING;
  }
  __syncthreads();
  if (t == 0) {
    int run = 0;
#pragma unroll
    for (int k = 0; k < KP; k++)
      run |= srun[k];
    st->running = run;
  }
}

// --------------------------------------------------------------------------
// Launchers (C ABI).  kp: 2, 4 or 8.
// --------------------------------------------------------------------------
template <int KP, bool RES>
static void spmm_launch(unsigned lanes, unsigned g, unsigned n, const int *offs, const int *cols, const double *vals,
                        const double *x, double *y, const double *bres, double *partials,
                        const struct lsb_mrhs_state *st, hipStream_t s) {
  ROW_KERNEL_LAUNCH(lanes, (k_spmm_csr<L, KP, RES>), g, s, n, offs, cols, vals, x, y, bres, partials, st);
}

extern "C" {

void lsb_k_mrhs_pack(unsigned n, unsigned kp, unsigned nrhs, const int *perm, const double *src, size_t ld,
                     double *dst, void *stream) {
  k_mrhs_pack<<<sweep_grid(n, kp), WG, 0, (hipStream_t)stream>>>(n, kshift_of(kp), nrhs, perm, src, ld, dst);
}

void lsb_k_mrhs_unpack(unsigned n, unsigned kp, unsigned nrhs, const int *perm, const double *src, double *dst,
                       size_t ld, void *stream) {
  k_mrhs_unpack<<<sweep_grid(n, kp), WG, 0, (hipStream_t)stream>>>(n, kshift_of(kp), nrhs, perm, src, dst, ld);
}

unsigned lsb_k_spmm_grid(unsigned n, unsigned lanes) {
  return lsb_k_spmv_grid(LSB_SPMV_SUBWAVE, n, 0, row_lanes(lanes), 0);
}

void lsb_k_spmm_csr(unsigned kp, unsigned n, const int *offs, const int *cols, const double *vals, unsigned lanes,
                    const double *x, double *y, const double *bres, double *partials, unsigned *npartials,
                    const struct lsb_mrhs_state *st, void *stream) {
  const unsigned L = row_lanes(lanes), g = lsb_k_spmm_grid(n, L);
  if (npartials)
    *npartials = g;
  if (bres)
    KP_DISPATCH(kp, (spmm_launch<KP, true>(L, g, n, offs, cols, vals, x, y, bres, partials, st, (hipStream_t)stream)));
  else
    KP_DISPATCH(kp, (spmm_launch<KP, false>(L, g, n, offs, cols, vals, x, y, bres, partials, st, (hipStream_t)stream)));
}

void lsb_k_mrhs_init(unsigned kp, unsigned n, const double *b, const double *dinv, double dc, double *x, double *r,
                     double *p, double *partials2, unsigned *npartials, void *stream) {
  const unsigned g = sweep_grid(n, kp);
  *npartials = g;
  KP_DISPATCH(kp, (k_mrhs_init<KP><<<g, WG, 0, (hipStream_t)stream>>>(n, b, dinv, dc, x, r, p, partials2)));
}

void lsb_k_amg_mrhs_init(unsigned kp, unsigned n, const double *b, double *x, double *r, void *stream) {
  KP_DISPATCH(kp, (k_amg_mrhs_init<KP><<<sweep_grid(n, kp), WG, 0, (hipStream_t)stream>>>(n, b, x, r)));
}

void lsb_k_amg_mrhs_init_p(unsigned kp, unsigned n, const double *b, const double *z, double *p, double *partials2,
                           unsigned *npartials, void *stream) {
  const unsigned g = sweep_grid(n, kp);
  *npartials = g;
  KP_DISPATCH(kp, (k_amg_dot2_m<KP, true><<<g, WG, 0, (hipStream_t)stream>>>(n, b, z, p, partials2, NULL)));
}

void lsb_k_amg_dot2_m(unsigned kp, unsigned n, const double *r, const double *z, double *records,
                      unsigned *nrecords, const struct lsb_mrhs_state *st, void *stream) {
  const unsigned g = sweep_grid(n, kp);
  *nrecords = g;
  KP_DISPATCH(kp, (k_amg_dot2_m<KP, false><<<g, WG, 0, (hipStream_t)stream>>>(n, r, z, NULL, records, st)));
}

void lsb_k_mrhs_init_state(unsigned kp, struct lsb_mrhs_state *st, const double *partials2, unsigned nparts,
                           const double *bb_parts, unsigned nbb, double tol, int maxit, void *stream) {
  KP_DISPATCH(kp, (k_mrhs_init_state<KP><<<1, WG, 0, (hipStream_t)stream>>>(st, partials2, nparts, bb_parts, nbb, tol,
                                                                            maxit)));
}

void lsb_k_mrhs_update_xr(unsigned kp, unsigned n, const double *p, const double *q, const double *dinv, double dc,
                          double *x, double *r, struct lsb_mrhs_state *st, int parity, const double *pq_parts,
                          unsigned npq, double *partials2, unsigned *npartials, void *stream) {
  const unsigned g = sweep_grid(n, kp);
  *npartials = g;
  KP_DISPATCH(kp, (k_mrhs_update_xr<KP, false><<<g, WG, 0, (hipStream_t)stream>>>(n, p, q, dinv, dc, x, r, st, parity,
                                                                                  pq_parts, npq, partials2)));
}

void lsb_k_amg_mrhs_update_xr(unsigned kp, unsigned n, const double *p, const double *q, double *x, double *r,
                              struct lsb_mrhs_state *st, int parity, const double *pq_parts, unsigned npq,
                              void *stream) {
  KP_DISPATCH(kp, (k_mrhs_update_xr<KP, true><<<sweep_grid(n, kp), WG, 0, (hipStream_t)stream>>>(
                      n, p, q, NULL, 0.0, x, r, st, parity, pq_parts, npq, NULL)));
}

void lsb_k_mrhs_update_p(unsigned kp, unsigned n, const double *r, const double *dinv, double dc, double *p,
                         struct lsb_mrhs_state *st, int parity, const double *parts2, unsigned nparts2,
                         void *stream) {
  const unsigned g = sweep_grid(n, kp);
  KP_DISPATCH(kp, (k_mrhs_update_p<KP, false><<<g, WG, 0, (hipStream_t)stream>>>(n, r, dinv, dc, p, st, parity, parts2,
                                                                                 nparts2)));
}

void lsb_k_amg_mrhs_update_p(unsigned kp, unsigned n, const double *z, double *p, struct lsb_mrhs_state *st,
                             int parity, const double *parts2, unsigned nparts2, void *stream) {
  KP_DISPATCH(kp, (k_mrhs_update_p<KP, true><<<sweep_grid(n, kp), WG, 0, (hipStream_t)stream>>>(
                      n, z, NULL, 0.0, p, st, parity, parts2, nparts2)));
}

void lsb_k_mrhs_restart(unsigned kp, unsigned n, const double *q, const double *dinv, double dc, double *r,
                        double *p, const struct lsb_mrhs_state *st, const double *rr_parts, unsigned nrr, int more,
                        double *partials, unsigned *npartials, void *stream) {
  const unsigned g = sweep_grid(n, kp);
  *npartials = g;
  KP_DISPATCH(kp, (k_mrhs_restart<KP><<<g, WG, 0, (hipStream_t)stream>>>(n, q, dinv, dc, r, p, st, rr_parts, nrr,
                                                                         more, partials)));
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

void lsb_k_mrhs_restart_state(unsigned kp, struct lsb_mrhs_state *st, const double *rr_parts, unsigned nrr,
                              const double *rz_parts, unsigned nrz, int more, void *stream) {
  KP_DISPATCH(kp, (k_mrhs_restart_state<KP><<<1, WG, 0, (hipStream_t)stream>>>(st, rr_parts, nrr, rz_parts, nrz,
                                                                               more)));
}

} // extern "C"
