// gfx950 (MI355X, CDNA4) BLAS-1, reduction, Jacobi, permutation and PCG sweep
// kernels of the lsbench HIP backend + their C-ABI launchers; the SpMV kernels
// and the two-launch PCG iteration's z-column kernels are in hip_kernels.hip.
// Kernel inventory = SURVEY.md section 8 (a2):
//   a2-2  dot, nrm2           two-stage, fixed-order => run-to-run identical
//   a2-3  axpy, xpay          scalars read from HBM, no host sync
//   a2-4  jacobi setup/apply/sweep
//   a2-5  fused PCG sweeps    (x,r update + r.z + r.r) and (p update)
#include "hip_kcommon.h"

// --------------------------------------------------------------------------
// a2-2  second stage of every reduction: one workgroup, fixed order.
// out[k] = sum over records of parts[i*width+k]   (sqrt'ed for nrm2)
// --------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void k_reduce_final(
    const double *__restrict__ parts, unsigned nparts, unsigned width,
    double *__restrict__ out, int take_sqrt,
    const lsb_pcg_state *__restrict__ st) {
  if (st && st->status)
    return;
  __shared__ double sred[4];
  for (unsigned k = 0; k < width; k++) {
    double v[1] = {0.0};
    for (unsigned i = threadIdx.x; i < nparts; i += WG)
      v[0] += parts[(size_t)i * width + k];
    wg_sum<1>(v, sred);
    if (threadIdx.x == 0)
      out[k] = take_sqrt ? sqrt(v[0]) : v[0];
  }
}

// two of those in one launch (the RCCL path of the single-reduction iteration
// needs the SpMV's and the sweep's partial sums reduced before ONE all-reduce)
__global__ __launch_bounds__(WG) void k_reduce_final2(
    const double *__restrict__ pa, unsigned na, unsigned wa, double *__restrict__ outa,
    const double *__restrict__ pb, unsigned nb, unsigned wb, double *__restrict__ outb,
    const lsb_pcg_state *__restrict__ st) {
  if (st && st->status)
    return;
  __shared__ double sred[4];
  for (unsigned k = 0; k < wa + wb; k++) {
    const bool a = k < wa;
    const double *p = a ? pa : pb;
    const unsigned n = a ? na : nb, w = a ? wa : wb, c = a ? k : k - wa;
    double v[1] = {0.0};
    for (unsigned i = threadIdx.x; i < n; i += WG)
      v[0] += p[(size_t)i * w + c];
    wg_sum<1>(v, sred);
    if (threadIdx.x == 0)
      (a ? outa : outb)[c] = v[0];
  }
}

// first stage of dot / nrm2 (b == a gives sum a_i^2)
__global__ __launch_bounds__(WG) void k_dot(unsigned n,
                                            const double *__restrict__ a,
                                            const double *__restrict__ b,
                                            double *__restrict__ partials) {
  __shared__ double sred[4];
  double v[1] = {0.0};
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n;
       i += (size_t)gridDim.x * WG)
    v[0] += a[i] * b[i];
  wg_sum<1>(v, sred);
  if (threadIdx.x == 0)
    partials[blockIdx.x] = v[0];
}

// --------------------------------------------------------------------------
// a2-3  axpy / xpay with the scalar in HBM
// --------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void k_axpy(unsigned n,
                                             const double *__restrict__ alpha,
                                             const double *__restrict__ x,
                                             double *__restrict__ y) {
  const double a = alpha[0];
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n;
       i += (size_t)gridDim.x * WG)
    y[i] += a * x[i];
}

__global__ __launch_bounds__(WG) void k_xpay(unsigned n,
                                             const double *__restrict__ beta,
                                             const double *__restrict__ x,
                                             double *__restrict__ y) {
  const double b = beta[0];
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n;
       i += (size_t)gridDim.x * WG)
    y[i] = x[i] + b * y[i];
}

// --------------------------------------------------------------------------
// a2-4  Jacobi
// --------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void k_jacobi_setup(
    unsigned n, unsigned row_begin, const int *__restrict__ offs,
    const int *__restrict__ cols, const double *__restrict__ vals,
    double *__restrict__ dinv, int *__restrict__ nzero) {
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n;
       i += (size_t)gridDim.x * WG) {
    const int want = (int)(i + row_begin);
    double d = 0.0;
    for (int j = offs[i]; j < offs[i + 1]; j++)
      if (cols[j] == want)
        d = vals[j];
    if (d != 0.0) {
      dinv[i] = 1.0 / d;
    } else {
      dinv[i] = 0.0;
      atomicAdd(nzero, 1);
    }
  }
}

// l1-Jacobi: dinv[i] = 1 / sum_j |S_ij| (the whole row, also its entries in
// other shards' columns: independent of the partition)
__global__ __launch_bounds__(WG) void k_l1_setup(unsigned n, const int *__restrict__ offs,
                                                 const double *__restrict__ vals,
                                                 double *__restrict__ dinv,
                                                 int *__restrict__ nzero) {
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n;
       i += (size_t)gridDim.x * WG) {
    double d = 0.0;
    for (int j = offs[i]; j < offs[i + 1]; j++)
      d += fabs(vals[j]);
    if (d != 0.0) {
      dinv[i] = 1.0 / d;
    } else {
      dinv[i] = 0.0;
      atomicAdd(nzero, 1);
    }
  }
}

__global__ __launch_bounds__(WG) void k_jacobi_apply(
    unsigned n, const double *__restrict__ dinv, const double *__restrict__ r,
    double *__restrict__ z) {
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n;
       i += (size_t)gridDim.x * WG)
    z[i] = dinv[i] * r[i];
}

// x <- x + w * dinv .* (b - ax)      (ax = Op x from a preceding SpMV)
__global__ __launch_bounds__(WG) void k_jacobi_sweep(
    unsigned n, double w, const double *__restrict__ dinv,
    const double *__restrict__ b, const double *__restrict__ ax,
    double *__restrict__ x) {
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n;
       i += (size_t)gridDim.x * WG)
    x[i] += w * dinv[i] * (b[i] - ax[i]);
}

// dst[i] = src[perm[i]]  /  dst[perm[i]] = src[i]   (reordering, perm[new] = old)
__global__ __launch_bounds__(WG) void k_perm_gather(unsigned n, const int *__restrict__ perm,
                                                    const double *__restrict__ src,
                                                    double *__restrict__ dst) {
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    const int j = perm[i]; // -1: a pad row of a line-padded grid (lsb_csr_pad_lines)
    dst[i] = j >= 0 ? src[j] : 0.0;
  }
}

__global__ __launch_bounds__(WG) void k_perm_scatter(unsigned n, const int *__restrict__ perm,
                                                     const double *__restrict__ src,
                                                     double *__restrict__ dst) {
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG) {
    const int j = perm[i];
    if (j >= 0)
      dst[j] = src[i];
  }
}

__global__ __launch_bounds__(WG) void k_fill_index(unsigned n, unsigned first,
                                                   double *__restrict__ v) {
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n;
       i += (size_t)gridDim.x * WG)
    v[i] = (double)(i + first);
}

// --------------------------------------------------------------------------
// a2-5  fused PCG sweeps.  Vector loads are 16 B/lane (double2) when every
// operand is 16-B aligned, 8 B/lane otherwise (a shard that starts on an odd
// row); the tail element, if any, is handled by the last thread.
// --------------------------------------------------------------------------

// x = 0, r = b, p = dinv.*b ; partials (r.z, b.b)
template <bool V2>
__global__ __launch_bounds__(WG) void k_pcg_init(
    unsigned n, const double *__restrict__ b, const double *__restrict__ dinv, double dc,
    double *__restrict__ x, double *__restrict__ r, double *__restrict__ p,
    double *__restrict__ partials2) {
  __shared__ double sred[8];
  double acc[2] = {0.0, 0.0};
  const size_t gtid = (size_t)blockIdx.x * WG + threadIdx.x;
  const size_t gsz = (size_t)gridDim.x * WG;
  if (V2) {
    const size_t n2 = n / 2;
    const double2 *b2 = (const double2 *)b, *d2 = (const double2 *)dinv;
    double2 *x2 = (double2 *)x, *r2 = (double2 *)r, *p2 = (double2 *)p;
    for (size_t i = gtid; i < n2; i += gsz) {
      const double2 bv = b2[i], dv = dinv ? d2[i] : double2{dc, dc};
      double2 pv;
      pv.x = dv.x * bv.x, pv.y = dv.y * bv.y;
      x2[i] = make_double2(0.0, 0.0);
      r2[i] = bv;
      p2[i] = pv;
      acc[0] += bv.x * pv.x;
      acc[0] += bv.y * pv.y;
      acc[1] += bv.x * bv.x;
      acc[1] += bv.y * bv.y;
    }
    if ((n & 1) && gtid == gsz - 1) {
      const size_t i = n - 1;
      const double bv = b[i], pv = (dinv ? dinv[i] : dc) * bv;
      x[i] = 0.0, r[i] = bv, p[i] = pv;
      acc[0] += bv * pv, acc[1] += bv * bv;
    }
  } else {
    for (size_t i = gtid; i < n; i += gsz) {
      const double bv = b[i], pv = (dinv ? dinv[i] : dc) * bv;
      x[i] = 0.0, r[i] = bv, p[i] = pv;
      acc[0] += bv * pv, acc[1] += bv * bv;
    }
  }
  wg_sum<2>(acc, sred);
  if (threadIdx.x == 0) {
    partials2[2 * blockIdx.x + 0] = acc[0];
    partials2[2 * blockIdx.x + 1] = acc[1];
  }
}

// warm start: r0 = b - q with q = S x0 ; partials (r0.r0, b.b).  The two sums are formed by the same expression
// in the same order: where x0 = 0 (q = 0, r0 = b) they have the same bits.
template <bool V2>
__global__ __launch_bounds__(WG) void k_x0_start(
    unsigned n, const double *__restrict__ b, const double *__restrict__ q, double *__restrict__ r0,
    double *__restrict__ partials2) {
  __shared__ double sred[8];
  double acc[2] = {0.0, 0.0};
  const size_t gtid = (size_t)blockIdx.x * WG + threadIdx.x;
  const size_t gsz = (size_t)gridDim.x * WG;
  if (V2) {
    const size_t n2 = n / 2;
    const double2 *b2 = (const double2 *)b, *q2 = (const double2 *)q;
    double2 *r2 = (double2 *)r0;
    for (size_t i = gtid; i < n2; i += gsz) {
      const double2 bv = b2[i], qv = q2[i];
      double2 rv;
      rv.x = bv.x - qv.x, rv.y = bv.y - qv.y;
      r2[i] = rv;
      acc[0] += rv.x * rv.x;
      acc[0] += rv.y * rv.y;
      acc[1] += bv.x * bv.x;
      acc[1] += bv.y * bv.y;
    }
    if ((n & 1) && gtid == gsz - 1) {
      const size_t i = n - 1;
      const double bv = b[i], rv = bv - q[i];
      r0[i] = rv;
      acc[0] += rv * rv, acc[1] += bv * bv;
    }
  } else {
    for (size_t i = gtid; i < n; i += gsz) {
      const double bv = b[i], rv = bv - q[i];
      r0[i] = rv;
      acc[0] += rv * rv, acc[1] += bv * bv;
    }
  }
  wg_sum<2>(acc, sred);
  if (threadIdx.x == 0) {
    partials2[2 * blockIdx.x + 0] = acc[0];
    partials2[2 * blockIdx.x + 1] = acc[1];
  }
}

// opts.verify behind a warm start: q = S x - b and the partials of q.q off the shard's CSR arrays (global column
// ids into the gather vector), L lanes per row, with every product's and every addition's rounding error carried
// along (two_prod through fma, two_sum; the butterfly folds (sum, error) pairs) -- k_spmm_csr<L, KP, true>'s scheme
// for one column: b - S x as if formed in twice the working precision, then rounded.  Where the recurrence has
// converged to 1e-13 an fp64 S x is mostly its own rounding (tests/xn3b_A_18.txt: 1 % of the residual).
__device__ __forceinline__ void two_sum1(double a, double b, double &s, double &e) {
#pragma clang fp contract(off)
  s = a + b;
  const double bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}

template <int L>
__global__ __launch_bounds__(WG) void k_resid_csr2(unsigned n, unsigned rows_per_wg, const int *__restrict__ offs,
                                                   const int *__restrict__ cols, const double *__restrict__ vals,
                                                   const double *__restrict__ xfull, const double *__restrict__ b,
                                                   double *__restrict__ q, double *__restrict__ partials) {
  constexpr unsigned SLOTS = WG / L;
  __shared__ double sred[4];
  const unsigned tid = threadIdx.x, slot = tid / L, l = tid % L;
  const unsigned ra = min(blockIdx.x * rows_per_wg, n), rb = min(ra + rows_per_wg, n);
  double dot[1] = {0.0};
  for (unsigned base = ra; base < rb; base += SLOTS) {
    const unsigned r = base + slot;
    double a = 0.0, e = 0.0;
    if (r < rb) {
#pragma clang fp contract(off)
      for (int j = offs[r] + (int)l; j < offs[r + 1]; j += L) {
        const double v = vals[j], t = xfull[cols[j]];
        const double pr = v * t, pe = fma(v, t, -pr);
        double se;
        two_sum1(a, pr, a, se);
        e += pe + se;
      }
    }
#pragma unroll
    for (int off = L >> 1; off > 0; off >>= 1) { // both partners form the same sum and the same error
#pragma clang fp contract(off)
      const double ao = __shfl_xor(a, off, 64), eo = __shfl_xor(e, off, 64);
      double se;
      two_sum1(a, ao, a, se);
      e = (e + eo) + se;
    }
    if (r < rb && l == 0) {
#pragma clang fp contract(off)
      double t0, te;
      two_sum1(b[r], -a, t0, te);
      const double res = t0 + (te - e); // b - S x
      q[r] = -res;
      dot[0] = fma(res, res, dot[0]);
    }
  }
  wg_sum<1>(dot, sred);
  if (tid == 0)
    partials[blockIdx.x] = dot[0];
}

__global__ __launch_bounds__(WG) void k_pcg_init_state(
    lsb_pcg_state *__restrict__ st, const double *__restrict__ partials2,
    unsigned nparts, double tol, int maxit) {
  __shared__ double sred[8];
  double v[2];
  wg_sum_partials<2>(partials2, nparts, v, sred);
  if (threadIdx.x == 0) {
    st->rz[0] = v[0];
    st->rz[1] = 0.0;
    st->alpha[0] = st->alpha[1] = 0.0; // "no previous step" marker of k_cg1_update
    st->bb = v[1];
    st->thresh2 = tol * tol * v[1];
    st->rr = v[1];
    st->pq = 0.0;
    st->iters = 0;
    st->maxit = maxit;
    st->pad = 0; // "maxit-th update done, status pending" marker of k_cg1_update / k_pcg_col_px
    st->xpend = 0; // k_pcg_col_px: no x update pending
    // b == 0 => x = 0 is the solution; maxit == 0 => nothing to do
    st->status = (v[1] == 0.0) ? LSB_STATUS_CONVERGED
                               : (maxit <= 0 ? LSB_STATUS_MAXIT : LSB_STATUS_RUNNING);
  }
}

// 16-byte lane loads of the BLAS-1 sweeps.  NT = nontemporal: on MI355X a
// plain read-only stream tops out near 4.6-4.8 TB/s while the same loop with
// nontemporal loads reads 6.1-6.2 TB/s (tools/spmv_lab.hip, "read-only" probes);
// a 5-in/2-out sweep shaped like k_pcg_update_xr gains 27 %.
typedef double d2v __attribute__((ext_vector_type(2)));
template <bool NT>
__device__ __forceinline__ d2v ld2(const d2v *p) {
  if (NT)
    return __builtin_nontemporal_load(p);
  return *p;
}
// Stores of vectors nobody reads before the NEXT sweep (x; in the single-
// reduction form also p, s, r): nontemporal, so that they do not sit as dirty
// lines in L2 / Infinity Cache while the SpMV that follows streams the matrix.
// Jacobi diagonal: a vector, or -- d2 == nullptr -- ONE value for every row (an
// operator with a constant diagonal: the preconditioner is a scaling and its
// vector need not be read; same arithmetic, the factor comes from a register).
template <bool NT>
__device__ __forceinline__ d2v ldd(const d2v *d2, size_t i, double dc) {
  if (!d2)
    return d2v{dc, dc};
  return ld2<NT>(d2 + i);
}
template <bool NT>
__device__ __forceinline__ void st2(d2v *p, d2v v) {
  if (NT)
    __builtin_nontemporal_store(v, p);
  else
    *p = v;
}

// alpha = rz/pq ; x += alpha p ; r -= alpha q ; partials (r.dinv.r, r.r)
// NTX / NTPQ / NTR: which operands are loaded nontemporal -- x (also stored so), p and q (and the
// Jacobi diagonal), r.  Which of them should bypass the caches is a matter of what the NEXT launches
// read again (LSBENCH_HIP_BLAS1_NT is the mask: bit 0 x, 1 p and q, 2 r here; 3 r, 4 p in
// k_pcg_update_p; 1 = all of them, the setting measured in rounds 1 and 2).
template <bool V2, bool NTX, bool NTPQ, bool NTR>
__global__ __launch_bounds__(WG) void k_pcg_update_xr(
    unsigned n, const double *__restrict__ p, const double *__restrict__ q,
    const double *__restrict__ dinv, double dc, double *__restrict__ x,
    double *__restrict__ r, lsb_pcg_state *__restrict__ st, int parity,
    const double *__restrict__ pq_parts, unsigned npq,
    double *__restrict__ partials2) {
  __shared__ double sred[8];
  const size_t gtid = (size_t)blockIdx.x * WG + threadIdx.x;
  const size_t gsz = (size_t)gridDim.x * WG;
  const size_t n2 = n / 2;
  const d2v *p2 = (const d2v *)p, *q2 = (const d2v *)q, *d2 = (const d2v *)dinv;
  d2v *x2 = (d2v *)x, *r2 = (d2v *)r;
  // Everything that does not depend on alpha is requested up front, so the
  // status word, the p.q partials, r.z and this lane's first operands are ONE
  // memory round trip, not four in a row (a small operator's sweep is nothing
  // but these latencies).
  const int stopped = st->status;
  const double rz = st->rz[parity];
  d2v pv = {0.0, 0.0}, qv = pv, dv = pv, xv = pv, rv = pv;
  const bool first = V2 && gtid < n2;
  if (first) {
    pv = ld2<NTPQ>(p2 + gtid), qv = ld2<NTPQ>(q2 + gtid), dv = ldd<NTPQ>(d2, gtid, dc);
    xv = ld2<NTX>(x2 + gtid), rv = ld2<NTR>(r2 + gtid);
  }
  double pqv[1];
  wg_sum_partials<1>(pq_parts, npq, pqv, sred);
  if (stopped)
    return;
  const double pq = pqv[0];
  if (!(pq != 0.0) || !isfinite(pq)) { // same decision in every workgroup
    if (blockIdx.x == 0 && threadIdx.x == 0)
      st->status = LSB_STATUS_BREAKDOWN;
    return;
  }
  const double alpha = rz / pq;
  if (blockIdx.x == 0 && threadIdx.x == 0)
    st->pq = pq;
  double acc[2] = {0.0, 0.0};
  if (V2) {
    if (first) {
      size_t i = gtid;
      for (;;) {
        xv.x += alpha * pv.x, xv.y += alpha * pv.y;
        rv.x -= alpha * qv.x, rv.y -= alpha * qv.y;
        st2<NTX>(x2 + i, xv), r2[i] = rv;
        acc[0] += rv.x * (dv.x * rv.x);
        acc[0] += rv.y * (dv.y * rv.y);
        acc[1] += rv.x * rv.x;
        acc[1] += rv.y * rv.y;
        i += gsz;
        if (i >= n2)
          break;
        pv = ld2<NTPQ>(p2 + i), qv = ld2<NTPQ>(q2 + i), dv = ldd<NTPQ>(d2, i, dc);
        xv = ld2<NTX>(x2 + i), rv = ld2<NTR>(r2 + i);
      }
    }
    if ((n & 1) && gtid == gsz - 1) {
      const size_t i = n - 1;
      x[i] += alpha * p[i];
      const double rs = r[i] - alpha * q[i];
      r[i] = rs;
      acc[0] += rs * ((dinv ? dinv[i] : dc) * rs), acc[1] += rs * rs;
    }
  } else {
    for (size_t i = gtid; i < n; i += gsz) {
      x[i] += alpha * p[i];
      const double rs = r[i] - alpha * q[i];
      r[i] = rs;
      acc[0] += rs * ((dinv ? dinv[i] : dc) * rs), acc[1] += rs * rs;
    }
  }
  wg_sum<2>(acc, sred);
  if (threadIdx.x == 0) {
    partials2[2 * blockIdx.x + 0] = acc[0];
    partials2[2 * blockIdx.x + 1] = acc[1];
  }
}

// (rz', rr) = sum partials ; stop test ; beta = rz'/rz ; p = dinv.*r + beta p
// X2: a lane keeps TWO 16-byte pairs per operand in flight (rows i and i + grid).  With one
// pair a lane has 32 bytes on their way (r and p; the constant diagonal is a register) --
// 2048 workgroups x 256 lanes x 32 B = 16.8 MB, about what 8 TB/s x 2 us of latency needs, and
// the sweep ran at 0.73 of peak where its five-operand sibling k_pcg_update_xr (64-80 B per
// lane) reaches 0.84 (profiles/r02_trace_kernel_stats.csv).
template <bool V2, bool NTR, bool NTP, bool X2>
__global__ __launch_bounds__(WG) void k_pcg_update_p(
    unsigned n, const double *__restrict__ r, const double *__restrict__ dinv, double dc,
    const double *pin, double *p, lsb_pcg_state *__restrict__ st, int parity,
    const double *__restrict__ parts2, unsigned nparts2) {
  // pin: where the previous direction is read from (== p, or the other buffer
  // of the launch-bound path that folds this update into the SpMV)
  __shared__ double sred[8];
  const size_t gtid = (size_t)blockIdx.x * WG + threadIdx.x;
  const size_t gsz = (size_t)gridDim.x * WG;
  const size_t n2 = n / 2;
  const d2v *r2 = (const d2v *)r, *d2 = (const d2v *)dinv;
  d2v *p2 = (d2v *)p;
  const d2v *pi2 = (const d2v *)pin;
  // as in k_pcg_update_xr: one round trip for status, scalars and operands
  const int stopped = st->status;
  const double rz_old = st->rz[parity], thresh2 = st->thresh2;
  if (blockIdx.x == 0 && threadIdx.x == 0)
    st->xpend = 0; // (two-launch column form: k_pcg_xfix, the launch before this one, has applied it; nobody
                   // reads the word in this launch)
  d2v rv = {0.0, 0.0}, dv = rv, pv = rv, rw = rv, dw = rv, pw = rv;
  const bool first = V2 && gtid < n2;
  bool second = X2 && V2 && gtid + gsz < n2;
  if (first)
    rv = ld2<NTR>(r2 + gtid), dv = ldd<NTR>(d2, gtid, dc), pv = ld2<NTP>(pi2 + gtid);
  if (second)
    rw = ld2<NTR>(r2 + gtid + gsz), dw = ldd<NTR>(d2, gtid + gsz, dc), pw = ld2<NTP>(pi2 + gtid + gsz);
  double v[2];
  wg_sum_partials<2>(parts2, nparts2, v, sred);
  if (stopped)
    return;
  const double rz_new = v[0], rr = v[1];
  const bool conv = rr <= thresh2;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    // only this thread touches iters/rr/rz[parity^1]/status in this launch
    const int it = st->iters + 1;
    st->iters = it;
    st->rr = rr;
    st->rz[parity ^ 1] = rz_new;
    if (conv)
      st->status = LSB_STATUS_CONVERGED;
    else if (it >= st->maxit)
      st->status = LSB_STATUS_MAXIT;
  }
  if (conv)
    return;
  const double beta = rz_new / rz_old;
  if (V2) {
    if (first) {
      size_t i = gtid;
      const size_t step = X2 ? 2 * gsz : gsz;
      for (;;) {
        pv.x = pnew_of(dv.x, rv.x, beta, pv.x); // one expression for every kernel that forms p
        pv.y = pnew_of(dv.y, rv.y, beta, pv.y);
        p2[i] = pv;
        if (X2 && second) {
          pw.x = pnew_of(dw.x, rw.x, beta, pw.x);
          pw.y = pnew_of(dw.y, rw.y, beta, pw.y);
          p2[i + gsz] = pw;
        }
        i += step;
        if (i >= n2)
          break;
        rv = ld2<NTR>(r2 + i), dv = ldd<NTR>(d2, i, dc), pv = ld2<NTP>(pi2 + i);
        if (X2) {
          second = i + gsz < n2;
          if (second)
            rw = ld2<NTR>(r2 + i + gsz), dw = ldd<NTR>(d2, i + gsz, dc), pw = ld2<NTP>(pi2 + i + gsz);
        }
      }
    }
    if ((n & 1) && gtid == gsz - 1)
      p[n - 1] = pnew_of(dinv ? dinv[n - 1] : dc, r[n - 1], beta, pin[n - 1]);
  } else {
    for (size_t i = gtid; i < n; i += gsz)
      p[i] = pnew_of(dinv ? dinv[i] : dc, r[i], beta, pin[i]);
  }
}

// --------------------------------------------------------------------------
// Single-reduction CG (Chronopoulos & Gear 1989), LSB_KRYLOV_PCG1: the same
// Krylov iterates as PCG in exact arithmetic, arranged so that an iteration is
// TWO launches and ONE global reduction instead of three and two:
//     [this kernel]  beta = g'/g ; alpha = g' / (d - beta g'/alpha)
//                    p = u + beta p ; s = w + beta s ; x += alpha p ; r -= alpha s
//                    u = D^-1 r ; partials (g'' = r.u, r.r)
//     [SpMV]         w = S u ; partials d = w.u         (the fused-dot SpMV)
// with g' = r.u and r.r taken from this kernel's own previous launch and
// d = w.u from the SpMV in between.  For launch-latency-bound operators that is
// 2/3 of the launches; across GPUs it is one all-reduce (3 doubles) per
// iteration instead of two.  Costs one more vector (s) and 96 n instead of 88 n
// bytes per iteration, so the large single-GPU case keeps the classic form.
// --------------------------------------------------------------------------
// UI ("implicit u"): the Jacobi diagonal is the constant dc, so u = dc r is not
// kept at all -- r itself lives in the gather vector, the SpMV in between
// delivers t = S r and r.t, and w = dc t, w.u = dc^2 r.t are formed here:
// 9 vector passes per sweep instead of 11 (u neither read nor written).
template <bool V2, bool NT, bool UI>
__global__ __launch_bounds__(WG) void k_cg1_update(
    unsigned n, double *__restrict__ u, const double *__restrict__ w,
    const double *__restrict__ dinv, double dc, double *__restrict__ p, double *__restrict__ sv,
    double *__restrict__ x, double *__restrict__ r, lsb_pcg_state *__restrict__ st,
    int parity, const double *__restrict__ parts_gr, unsigned ngr,
    const double *__restrict__ parts_d, unsigned nd, const lsb_ar_collect col,
    double *__restrict__ partials2) {
  __shared__ double sred[8];
  const size_t gtid = (size_t)blockIdx.x * WG + threadIdx.x;
  const size_t gsz = (size_t)gridDim.x * WG;
  const size_t n2 = n / 2;
  // `pend`: the previous launch was the maxit-th update.  That launch does NOT
  // publish LSB_STATUS_MAXIT itself: its workgroups read the status word on
  // entry, and one that started after the leader's store would skip its slice
  // of x/r/p/s (a mix of two iterates).  It raises st->pad instead, a word
  // nobody tests in that launch; THIS launch promotes it to the final status --
  // every workgroup sees pad = 1 (written one launch ago) and returns, whatever
  // it reads in the status word.
  const int stopped = st->status, pend = st->pad;
  const double g_old = st->rz[parity], a_old = st->alpha[parity], thresh2 = st->thresh2;
  d2v *u2 = (d2v *)u, *p2 = (d2v *)p, *s2 = (d2v *)sv, *x2 = (d2v *)x, *r2 = (d2v *)r;
  const d2v *w2 = (const d2v *)w, *d2 = (const d2v *)dinv;
  d2v uv = {0.0, 0.0}, wv = uv, dv = uv, pv = uv, sw = uv, xv = uv, rv = uv;
  const bool first = V2 && gtid < n2;
  if (first) {
    wv = ld2<NT>(w2 + gtid), dv = ldd<NT>(d2, gtid, dc);
    pv = ld2<NT>(p2 + gtid), sw = ld2<NT>(s2 + gtid), xv = ld2<NT>(x2 + gtid);
    // (the vector the SpMV gathers next -- r with the implicit u, else u -- is loaded the plain
    // way: loaded nontemporal it is gone from the caches when the SpMV wants it, 40 instead of
    // 25 us on the 10 M-row operator, as with p in k_pcg_update_p)
    rv = ld2 < NT && !UI > (r2 + gtid);
    if (UI)
      uv = dc * rv, wv = dc * wv;
    else
      uv = ld2<false>(u2 + gtid);
  }
  double gr[2], dd[1];
  if (col.mbox) {
    // sharded solve over the direct xGMI path: the SpMV launch in front of this
    // one sent this rank's sums to every rank; take w.u, r.u, r.r from the
    // mailbox (rank order: the same bits everywhere) -- hip_ar.h
    if (stopped)
      return;
    if (threadIdx.x < 64) {
      double v[3];
      const bool ok = ar_collect<false>(col.mbox, col.R, col.epoch, col.timeout, 3, v);
      if (threadIdx.x == 0)
        sred[0] = v[0], sred[1] = v[1], sred[2] = v[2], sred[3] = ok ? 1.0 : 0.0;
    }
    __syncthreads();
    dd[0] = sred[0], gr[0] = sred[1], gr[1] = sred[2];
    if (sred[3] == 0.0) { // a peer did not arrive: every workgroup that notices says so
      if (threadIdx.x == 0)
        __hip_atomic_store(&st->status, (int)LSB_STATUS_COMM, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
      return;
    }
  } else {
    wg_sum_partials<2>(parts_gr, ngr, gr, sred);
    wg_sum_partials<1>(parts_d, nd, dd, sred);
    if (stopped)
      return;
  }
  const double g_new = gr[0], rr = gr[1], delta = UI ? dc * dc * dd[0] : dd[0];
  const bool leader = blockIdx.x == 0 && threadIdx.x == 0;
  if (rr <= thresh2 || pend) { // r of the previous update meets the tolerance, or it was the last allowed
    if (leader)
      st->status = rr <= thresh2 ? LSB_STATUS_CONVERGED : LSB_STATUS_MAXIT, st->rr = rr;
    return;
  }
  double beta = 0.0, alpha;
  if (a_old == 0.0) { // first iteration of the solve (k_pcg_init_state zeroes alpha)
    alpha = g_new / delta;
  } else {
    beta = g_new / g_old;
    alpha = g_new / (delta - beta * g_new / a_old);
  }
  if (!isfinite(alpha) || alpha == 0.0) { // same decision in every workgroup
    if (leader)
      st->status = LSB_STATUS_BREAKDOWN;
    return;
  }
  if (leader) {
    const int it = st->iters + 1;
    st->iters = it;
    st->rr = rr;
    st->pq = delta;
    st->rz[parity ^ 1] = g_new;
    st->alpha[parity ^ 1] = alpha;
    if (it >= st->maxit)
      st->pad = 1; // promoted to LSB_STATUS_MAXIT / CONVERGED by the next launch (see `pend`)
  }
  double acc[2] = {0.0, 0.0};
  if (V2) {
    if (first) {
      size_t i = gtid;
      for (;;) {
        pv.x = uv.x + beta * pv.x, pv.y = uv.y + beta * pv.y;
        sw.x = wv.x + beta * sw.x, sw.y = wv.y + beta * sw.y;
        xv.x += alpha * pv.x, xv.y += alpha * pv.y;
        rv.x -= alpha * sw.x, rv.y -= alpha * sw.y;
        uv.x = dv.x * rv.x, uv.y = dv.y * rv.y;
        st2<NT>(p2 + i, pv), st2<NT>(s2 + i, sw), st2<NT>(x2 + i, xv);
        if (UI) {
          r2[i] = rv; // the SpMV gathers it next: keep it cached
        } else {
          st2<NT>(r2 + i, rv);
          u2[i] = uv;
        }
        acc[0] += rv.x * uv.x;
        acc[0] += rv.y * uv.y;
        acc[1] += rv.x * rv.x;
        acc[1] += rv.y * rv.y;
        i += gsz;
        if (i >= n2)
          break;
        wv = ld2<NT>(w2 + i), dv = ldd<NT>(d2, i, dc);
        pv = ld2<NT>(p2 + i), sw = ld2<NT>(s2 + i), xv = ld2<NT>(x2 + i);
        rv = ld2 < NT && !UI > (r2 + i);
        if (UI)
          uv = dc * rv, wv = dc * wv;
        else
          uv = ld2<false>(u2 + i);
      }
    }
    if ((n & 1) && gtid == gsz - 1) {
      const size_t i = n - 1;
      const double ui0 = UI ? dc * r[i] : u[i], wi = UI ? dc * w[i] : w[i];
      const double pi = ui0 + beta * p[i], si = wi + beta * sv[i];
      p[i] = pi, sv[i] = si;
      x[i] += alpha * pi;
      const double ri = r[i] - alpha * si, ui = (dinv ? dinv[i] : dc) * ri;
      r[i] = ri;
      if (!UI)
        u[i] = ui;
      acc[0] += ri * ui, acc[1] += ri * ri;
    }
  } else {
    for (size_t i = gtid; i < n; i += gsz) {
      const double ui0 = UI ? dc * r[i] : u[i], wi = UI ? dc * w[i] : w[i];
      const double pi = ui0 + beta * p[i], si = wi + beta * sv[i];
      p[i] = pi, sv[i] = si;
      x[i] += alpha * pi;
      const double ri = r[i] - alpha * si, ui = (dinv ? dinv[i] : dc) * ri;
      r[i] = ri;
      if (!UI)
        u[i] = ui;
      acc[0] += ri * ui, acc[1] += ri * ri;
    }
  }
  wg_sum<2>(acc, sred);
  if (threadIdx.x == 0) {
    partials2[2 * blockIdx.x + 0] = acc[0];
    partials2[2 * blockIdx.x + 1] = acc[1];
  }
}

// Virtual-rank stand-in for the all-reduce: `nshard` shards on ONE device keep
// their scalars at base[q*stride + off .. +cnt); sum over q in rank order and
// hand every shard the same bits.
__global__ void k_vreduce(double *__restrict__ base, unsigned stride,
                          unsigned nshard, unsigned off, unsigned cnt) {
  const unsigned t = threadIdx.x;
  if (t < cnt) {
    double s = 0.0;
    for (unsigned q = 0; q < nshard; q++)
      s += base[(size_t)q * stride + off + t];
    for (unsigned q = 0; q < nshard; q++)
      base[(size_t)q * stride + off + t] = s;
  }
}

// the x update a run's last k_pcg_col_r left pending (no k_pcg_col_px came behind it, or that one
// found the solve converged): x += alpha p with p in the buffer st->xpend names.  Runs whatever the
// status; the stand-alone k_pcg_update_p behind it clears st->xpend.
__global__ __launch_bounds__(WG) void k_pcg_xfix(unsigned n, const double *__restrict__ p0, const double *__restrict__ p1,
                                                 double *__restrict__ x, const lsb_pcg_state *__restrict__ st) {
  const int pend = st->xpend;
  if (!pend)
    return;
  const double alpha = st->alpha[0], alpha2 = st->alpha[1];
  if (pend <= 2) { // one update behind: the direction is in buffer pend - 1
    const double *__restrict__ p = pend == 1 ? p0 : p1;
    for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG)
      x[i] += alpha * p[i];
  } else { // two: the last direction in buffer pend - 3, the one before it in the other
    const double *__restrict__ p = pend == 3 ? p0 : p1, *__restrict__ pp = pend == 3 ? p1 : p0;
    for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += (size_t)gridDim.x * WG)
      x[i] = (x[i] + alpha2 * pp[i]) + alpha * p[i];
  }
}

// --------------------------------------------------------------------------
// Launchers (C ABI)
// --------------------------------------------------------------------------
extern "C" {

unsigned lsb_k_blas1_grid(unsigned n) {
  // 16 B/lane => WG*2 elements per workgroup per trip.  Up to 256 workgroups
  // one trip each (small operators: all latency); beyond that four trips per
  // lane before the grid grows -- every workgroup of the NEXT kernel re-reduces
  // this kernel's partial sums, so a grid of 2048 on a 1 M-row shard costs more
  // in its consumers than it gains (1.25 M rows: sweep 26.5 -> 20.8 us); cap at
  // MAX_PARTIALS.
  unsigned g = div_up(n, WG * 2);
  if (g > 256) {
    g = div_up(n, WG * 2 * 4);
    if (g < 256)
      g = 256;
  }
  // ... and at three workgroups per CU: beyond that the sweeps get SLOWER the more of them stream
  // at once -- round 3, iteration of the 64 M-row 7-point operator (vectors of 512 MB: nothing
  // comes out of the Infinity Cache) 1211-1238 us with 2048 workgroups, 1075-1077 us with 768
  // (256 / 512 / 1024: 1081-1104 / 1082-1090 / 1103-1110), the 10 M-row 5-point one 140-142 ->
  // 136-137 us; y = 4 x over 512 MB vectors: 178 us with 1024 workgroups, 204-207 us with
  // 2048 / 4096 (profiles/r03_sweep_grid.txt).
  if (g > LSB_STREAM_GRID_CAP)
    g = LSB_STREAM_GRID_CAP;
  return g ? g : 1;
}

void lsb_k_reduce_final(const double *partials, unsigned nparts, unsigned width,
                        double *out, int take_sqrt,
                        const struct lsb_pcg_state *st, void *stream) {
  k_reduce_final<<<1, WG, 0, (hipStream_t)stream>>>(partials, nparts, width, out,
                                                    take_sqrt, st);
}

void lsb_k_reduce_final2(const double *pa, unsigned na, unsigned wa, double *outa,
                         const double *pb, unsigned nb, unsigned wb, double *outb,
                         const struct lsb_pcg_state *st, void *stream) {
  k_reduce_final2<<<1, WG, 0, (hipStream_t)stream>>>(pa, na, wa, outa, pb, nb, wb, outb, st);
}

void lsb_k_dot(unsigned n, const double *a, const double *b, double *partials,
               unsigned *npartials, void *stream) {
  unsigned g = div_up(n ? n : 1, WG * 4);
  if (g > LSB_STREAM_GRID_CAP)
    g = LSB_STREAM_GRID_CAP;
  *npartials = g;
  k_dot<<<g, WG, 0, (hipStream_t)stream>>>(n, a, b, partials);
}

static unsigned ew_grid(unsigned n) {
  unsigned g = div_up(n ? n : 1, WG * 4);
  return g > LSB_STREAM_GRID_CAP ? LSB_STREAM_GRID_CAP : g;
}

void lsb_k_axpy(unsigned n, const double *alpha, const double *x, double *y,
                void *stream) {
  k_axpy<<<ew_grid(n), WG, 0, (hipStream_t)stream>>>(n, alpha, x, y);
}

void lsb_k_xpay(unsigned n, const double *beta, const double *x, double *y,
                void *stream) {
  k_xpay<<<ew_grid(n), WG, 0, (hipStream_t)stream>>>(n, beta, x, y);
}

void lsb_k_jacobi_setup(unsigned n, unsigned row_begin, const int *offs,
                        const int *cols, const double *vals, double *dinv,
                        int *nzero, void *stream) {
  k_jacobi_setup<<<ew_grid(n), WG, 0, (hipStream_t)stream>>>(n, row_begin, offs, cols,
                                                             vals, dinv, nzero);
}

void lsb_k_l1_setup(unsigned n, const int *offs, const double *vals, double *dinv, int *nzero,
                    void *stream) {
  k_l1_setup<<<ew_grid(n), WG, 0, (hipStream_t)stream>>>(n, offs, vals, dinv, nzero);
}

void lsb_k_jacobi_apply(unsigned n, const double *dinv, const double *r,
                        double *z, void *stream) {
  k_jacobi_apply<<<ew_grid(n), WG, 0, (hipStream_t)stream>>>(n, dinv, r, z);
}

void lsb_k_jacobi_sweep(unsigned n, double w, const double *dinv,
                        const double *b, const double *ax, double *x,
                        void *stream) {
  k_jacobi_sweep<<<ew_grid(n), WG, 0, (hipStream_t)stream>>>(n, w, dinv, b, ax, x);
}

void lsb_k_vreduce(double *base, unsigned stride, unsigned nshard, unsigned off,
                   unsigned cnt, void *stream) {
  k_vreduce<<<1, 64, 0, (hipStream_t)stream>>>(base, stride, nshard, off, cnt);
}

void lsb_k_perm_gather(unsigned n, const int *perm, const double *src, double *dst,
                       void *stream) {
  k_perm_gather<<<ew_grid(n), WG, 0, (hipStream_t)stream>>>(n, perm, src, dst);
}

void lsb_k_perm_scatter(unsigned n, const int *perm, const double *src, double *dst,
                        void *stream) {
  k_perm_scatter<<<ew_grid(n), WG, 0, (hipStream_t)stream>>>(n, perm, src, dst);
}

void lsb_k_fill_index(unsigned n, unsigned first, double *v, void *stream) {
  k_fill_index<<<ew_grid(n), WG, 0, (hipStream_t)stream>>>(n, first, v);
}

void lsb_k_pcg_init(unsigned n, const double *b, const double *dinv, double dc, double *x,
                    double *r, double *p, double *partials2,
                    unsigned *npartials, void *stream) {
  const unsigned g = lsb_k_blas1_grid(n);
  *npartials = g;
  const bool v2 = aligned16(b) && aligned16(dinv) && aligned16(x) && aligned16(r) && aligned16(p);
  const auto kern = v2 ? k_pcg_init<true> : k_pcg_init<false>;
  kern<<<g, WG, 0, (hipStream_t)stream>>>(n, b, dinv, dc, x, r, p, partials2);
}

void lsb_k_x0_start(unsigned n, const double *b, const double *q, double *r0, double *partials2,
                    unsigned *npartials, void *stream) {
  const unsigned g = lsb_k_blas1_grid(n);
  *npartials = g;
  const bool v2 = aligned16(b) && aligned16(q) && aligned16(r0);
  const auto kern = v2 ? k_x0_start<true> : k_x0_start<false>;
  kern<<<g, WG, 0, (hipStream_t)stream>>>(n, b, q, r0, partials2);
}

void lsb_k_resid_csr2(unsigned n, const int *offs, const int *cols, const double *vals, unsigned lanes,
                      const double *xfull, const double *b, double *q, double *partials, unsigned *npartials,
                      void *stream) {
  const unsigned slots = WG / row_lanes(lanes); // rows a workgroup works on at once
  unsigned g = div_up(n ? n : 1, 4 * slots);
  if (g > LSB_MAX_PARTIALS)
    g = LSB_MAX_PARTIALS;
  const unsigned rows_per_wg = round_up(div_up(n ? n : 1, g), slots);
  g = div_up(n ? n : 1, rows_per_wg);
  *npartials = g;
  LANES_DISPATCH(lanes, (k_resid_csr2<L><<<g, WG, 0, (hipStream_t)stream>>>(n, rows_per_wg, offs, cols, vals, xfull, b, q,
                                                                        partials)));
}

void lsb_k_pcg_init_state(struct lsb_pcg_state *st, const double *partials2,
                          unsigned nparts, double tol, int maxit,
                          void *stream) {
  k_pcg_init_state<<<1, WG, 0, (hipStream_t)stream>>>(st, partials2, nparts, tol, maxit);
}

/* nt: which operands of the sweeps are loaded nontemporal -- bits 0, 1, 2 here (x, p and q, r); 3, 4 in
 * lsb_k_pcg_update_p (r, p); 5 lsb_k_cg1_update (picked per solver at its creation, hip_pcg.c) */
void lsb_k_pcg_update_xr(unsigned n, const double *p, const double *q,
                         const double *dinv, double dc, double *x, double *r,
                         struct lsb_pcg_state *st, int parity,
                         const double *pq_parts, unsigned npq,
                         double *partials2, unsigned *npartials, unsigned nt, void *stream) {
  const unsigned g = lsb_k_blas1_grid(n);
  *npartials = g;
  static decltype(&k_pcg_update_xr<true, false, false, false>) const v2[8] = { /* [nt & 7] */
      k_pcg_update_xr<true, false, false, false>, k_pcg_update_xr<true, true, false, false>,
      k_pcg_update_xr<true, false, true, false>,  k_pcg_update_xr<true, true, true, false>,
      k_pcg_update_xr<true, false, false, true>,  k_pcg_update_xr<true, true, false, true>,
      k_pcg_update_xr<true, false, true, true>,   k_pcg_update_xr<true, true, true, true>};
  auto kern = k_pcg_update_xr<false, false, false, false>;
  if (aligned16(p) && aligned16(q) && aligned16(dinv) && aligned16(x) && aligned16(r))
    kern = v2[nt & 7];
  kern<<<g, WG, 0, (hipStream_t)stream>>>(n, p, q, dinv, dc, x, r, st, parity, pq_parts, npq, partials2);
}

void lsb_k_pcg_xfix(unsigned n, const double *p0, const double *p1, double *x, const struct lsb_pcg_state *st,
                    void *stream) {
  k_pcg_xfix<<<lsb_k_blas1_grid(n), WG, 0, (hipStream_t)stream>>>(n, p0, p1, x, st);
}

void lsb_k_cg1_update(unsigned n, double *u, const double *w, const double *dinv, double dc,
                      double *p,
                      double *s, double *x, double *r, struct lsb_pcg_state *st, int parity,
                      const double *parts_gr, unsigned ngr, const double *parts_d, unsigned nd,
                      const struct lsb_ar_collect *collect, double *partials2,
                      unsigned *npartials, unsigned nt, void *stream) {
  const unsigned g = lsb_k_blas1_grid(n);
  *npartials = g;
  lsb_ar_collect col;
  memset(&col, 0, sizeof col);
  if (collect)
    col = *collect;
  const bool v2 = aligned16(u) && aligned16(w) && aligned16(dinv) && aligned16(p) &&
                  aligned16(s) && aligned16(x) && aligned16(r);
  /* u == NULL: implicit u = dc r, r is the gather vector (needs the constant diagonal) */
  const bool ui = !u;
  if (ui && dinv)
    errx(EXIT_FAILURE, "lsb_k_cg1_update: implicit u needs a constant diagonal");
  auto kern = ui ? k_cg1_update<false, false, true> : k_cg1_update<false, false, false>;
  if (v2 && (nt & 32))
    kern = ui ? k_cg1_update<true, true, true> : k_cg1_update<true, true, false>;
  else if (v2)
    kern = ui ? k_cg1_update<true, false, true> : k_cg1_update<true, false, false>;
  kern<<<g, WG, 0, (hipStream_t)stream>>>(n, u, w, dinv, dc, p, s, x, r, st, parity, parts_gr, ngr, parts_d, nd,
                                          col, partials2);
}

void lsb_k_pcg_update_p(unsigned n, const double *r, const double *dinv, double dc,
                        const double *pin, double *p, struct lsb_pcg_state *st, int parity,
                        const double *parts2, unsigned nparts2, unsigned nt, void *stream) {
  const unsigned g = lsb_k_blas1_grid(n);
  const int x2 = 1; /* two pairs per operand in flight (one: 40.6 against 40.4 us, round 3 -- no difference) */
  static decltype(&k_pcg_update_p<true, false, false, false>) const v2[2][4] = { /* [big][(nt >> 3) & 3] */
      {k_pcg_update_p<true, false, false, false>, k_pcg_update_p<true, true, false, false>,
       k_pcg_update_p<true, false, true, false>, k_pcg_update_p<true, true, true, false>},
      {k_pcg_update_p<true, false, false, true>, k_pcg_update_p<true, true, false, true>,
       k_pcg_update_p<true, false, true, true>, k_pcg_update_p<true, true, true, true>}};
  auto kern = k_pcg_update_p<false, false, false, false>;
  if (aligned16(r) && aligned16(dinv) && aligned16(p) && aligned16(pin)) {
    const bool big = x2 && (size_t)n / 2 > (size_t)g * WG; /* a second pair exists at all */
    kern = v2[big][(nt >> 3) & 3];
  }
  kern<<<g, WG, 0, (hipStream_t)stream>>>(n, r, dinv, dc, pin, p, st, parity, parts2, nparts2);
}

} // extern "C"
