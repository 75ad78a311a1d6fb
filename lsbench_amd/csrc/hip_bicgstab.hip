// BiCGSTAB with right Jacobi preconditioning (LSB_KRYLOV_BICGSTAB) -- the method of the
// reference's one in-tree Krylov call site (BiCGSTAB + Jacobi, src/ginkgo.cpp:55-64;
// SURVEY.md section 8 a1-7), and the short-recurrence method for operators that are not
// symmetric: seven vectors whatever the iteration count, where GMRES(30) keeps 31.
//
//   p^ = D^-1 p ; v = Op p^ ; sigma = r^.v          SpMV with the fused dot, xdot = r^
//   alpha = rho/sigma ; s = r - alpha v ; ss = s.s   k_bcg_s   (s in place in r, s^ = D^-1 s)
//   t = Op s^ ; ts = t.s                             SpMV with the fused dot, xdot = s
//   tt = t.t                                         k_bcg_tt
//   half step if ss <= tol^2 bb: x += alpha p^       k_bcg_xr
//   omega = ts/tt ; x += alpha p^ + omega s^ ; r = s - omega t ; rr = r.r ; rho' = r^.r
//   stop test ; beta = (rho'/rho)(alpha/omega) ; p = r + beta (p - omega v) ; p^ = D^-1 p   k_bcg_p
//
// Four sweep launches and 20 vector passes per iteration beside the two SpMVs (18 where the
// Jacobi diagonal is one constant): k_bcg_s 5 (r v dinv in, r s^ out), k_bcg_tt 1, k_bcg_xr 8
// (x p^ s^ s t r^ in, x r out), k_bcg_p 6 (r p v dinv in, p p^ out).
//
// All scalars live in lsb_bcg_state on the device; the host never sees alpha, omega or beta.
// Every kernel returns at once when the status has left RUNNING.  The rules the PCG sweeps
// follow hold here too:
//   * a reduction is one partial per workgroup, summed again in fixed order by EVERY workgroup
//     of the consuming launch (wg_sum_partials): no atomics, the same bits run after run, and
//     every workgroup takes the same decision from the same numbers;
//   * a COEFFICIENT that workgroups read on entry is never written in the same launch: rho is
//     double-buffered by iteration parity, alpha / omega are written one launch before they
//     are read, iters and nspmv are the leader's alone.  The status word is the exception: every
//     workgroup reads it on entry and the leader may write it in the same launch, which is safe
//     only where a workgroup that sees the new value does what it would have done anyway --
//     BREAKDOWN and CONVERGED in k_bcg_s / k_bcg_xr / k_bcg_p are decided by every workgroup from
//     the same partials and none of them writes a vector then; MAXIT in k_bcg_p makes late
//     workgroups skip their part of p and p^, which nobody reads again (a run that ended in MAXIT
//     is never continued, and the restart of opts.verify forms p anew).  The half step is the
//     case that is NOT safe -- every workgroup must finish its part of x -- so k_bcg_xr raises
//     `half` instead, and the NEXT launch (k_bcg_p) turns it into LSB_STATUS_CONVERGED;
//   * one rounding rule: every update is an explicit fma chain, the same in the 16-byte and the
//     8-byte instantiation.
// No coefficient that is zero where it divides, or not finite, ever reaches a vector: the
// launch that finds one sets LSB_STATUS_BREAKDOWN and writes nothing.
#include "hip_kcommon.h"

typedef double b2v __attribute__((ext_vector_type(2)));
// loads of operands nobody reads again before they are overwritten: nontemporal (hip_sweeps.hip, ld2)
__device__ __forceinline__ b2v ldnt(const b2v *p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ b2v ldd2(const b2v *d2, size_t i, double dc) {
  return d2 ? ldnt(d2 + i) : b2v{dc, dc};
}

#define BCG_IDX                                                     \
  const size_t gtid = (size_t)blockIdx.x * WG + threadIdx.x;        \
  const size_t gsz = (size_t)gridDim.x * WG;                        \
  const size_t n2 = n / 2;                                          \
  const bool tail = (n & 1) && gtid == gsz - 1; /* the odd last element of the 16-byte form */ \
  (void)n2, (void)tail
#define BCG_LEADER (blockIdx.x == 0 && threadIdx.x == 0)

// x = 0 ; r = r^ = p = b ; p^ = D^-1 b ; partials of b.b (= rho)
template <bool V2>
__global__ __launch_bounds__(WG) void k_bcg_init(unsigned n, const double *__restrict__ b,
                                                 const double *__restrict__ dinv, double dc,
                                                 double *__restrict__ x, double *__restrict__ r,
                                                 double *__restrict__ rhat, double *__restrict__ p,
                                                 double *__restrict__ phat, double *__restrict__ partials) {
  __shared__ double sred[4];
  BCG_IDX;
  double acc[1] = {0.0};
  if (V2) {
    const b2v *d2 = (const b2v *)dinv;
    for (size_t i = gtid; i < n2; i += gsz) {
      const b2v bv = ((const b2v *)b)[i], dv = ldd2(d2, i, dc);
      ((b2v *)x)[i] = b2v{0.0, 0.0};
      ((b2v *)r)[i] = bv, ((b2v *)rhat)[i] = bv, ((b2v *)p)[i] = bv;
      ((b2v *)phat)[i] = b2v{dv.x * bv.x, dv.y * bv.y};
      acc[0] = fma(bv.y, bv.y, fma(bv.x, bv.x, acc[0]));
    }
  }
  for (size_t i = V2 ? (tail ? n - 1 : n) : gtid; i < n; i += gsz) {
    const double bv = b[i];
    x[i] = 0.0, r[i] = bv, rhat[i] = bv, p[i] = bv;
    phat[i] = (dinv ? dinv[i] : dc) * bv;
    acc[0] = fma(bv, bv, acc[0]);
  }
  wg_sum<1>(acc, sred);
  if (threadIdx.x == 0)
    partials[blockIdx.x] = acc[0];
}

// one workgroup: b.b starts the state (not gated: the state still holds the previous solve's status)
__global__ __launch_bounds__(WG) void k_bcg_init_state(lsb_bcg_state *__restrict__ st,
                                                       const double *__restrict__ parts, unsigned nparts,
                                                       double tol, int maxit) {
  __shared__ double sred[4];
  double v[1];
  wg_sum_partials<1>(parts, nparts, v, sred);
  if (threadIdx.x != 0)
    return;
  const double bb = v[0];
  st->c.bb = bb, st->c.thresh2 = tol * tol * bb, st->c.rr = bb;
  st->c.iters = 0, st->c.maxit = maxit;
  st->rho[0] = st->rho[1] = bb; // r^ = r0 = b
  st->alpha = st->omega = 0.0;
  st->half = st->nspmv = 0;
  // b == 0 => x = 0 is the solution; maxit == 0 => nothing to do
  st->c.status = bb == 0.0 ? LSB_STATUS_CONVERGED : (maxit <= 0 ? LSB_STATUS_MAXIT : LSB_STATUS_RUNNING);
}

// the restart of opts.verify: r = b - Op x (ax = Op x) ; r^ = p = r ; p^ = D^-1 r ; partials of r.r.
// Not gated: it runs on a state that says CONVERGED.
template <bool V2>
__global__ __launch_bounds__(WG) void k_bcg_restart(unsigned n, const double *__restrict__ b,
                                                    const double *__restrict__ ax,
                                                    const double *__restrict__ dinv, double dc,
                                                    double *__restrict__ r, double *__restrict__ rhat,
                                                    double *__restrict__ p, double *__restrict__ phat,
                                                    double *__restrict__ partials) {
  __shared__ double sred[4];
  BCG_IDX;
  double acc[1] = {0.0};
  if (V2) {
    const b2v *d2 = (const b2v *)dinv;
    for (size_t i = gtid; i < n2; i += gsz) {
      const b2v bv = ((const b2v *)b)[i], av = ((const b2v *)ax)[i], dv = ldd2(d2, i, dc);
      const b2v rv = {bv.x - av.x, bv.y - av.y};
      ((b2v *)r)[i] = rv, ((b2v *)rhat)[i] = rv, ((b2v *)p)[i] = rv;
      ((b2v *)phat)[i] = b2v{dv.x * rv.x, dv.y * rv.y};
      acc[0] = fma(rv.y, rv.y, fma(rv.x, rv.x, acc[0]));
    }
  }
  for (size_t i = V2 ? (tail ? n - 1 : n) : gtid; i < n; i += gsz) {
    const double rv = b[i] - ax[i];
    r[i] = rv, rhat[i] = rv, p[i] = rv;
    phat[i] = (dinv ? dinv[i] : dc) * rv;
    acc[0] = fma(rv, rv, acc[0]);
  }
  wg_sum<1>(acc, sred);
  if (threadIdx.x == 0)
    partials[blockIdx.x] = acc[0];
}

// one workgroup: the recomputed ||b - Op x||^2 decides -- converged (verified), or run on from it
// (more != 0: another restart is allowed), or not converged
__global__ __launch_bounds__(WG) void k_bcg_restart_state(lsb_bcg_state *__restrict__ st,
                                                          const double *__restrict__ parts, unsigned nparts,
                                                          int more) {
  __shared__ double sred[4];
  double v[1];
  wg_sum_partials<1>(parts, nparts, v, sred);
  if (threadIdx.x != 0)
    return;
  const double rr = v[0];
  st->c.rr = rr;
  st->rho[0] = st->rho[1] = rr; // r^ = r
  st->half = 0;
  st->c.status = rr <= st->c.thresh2                     ? LSB_STATUS_CONVERGED
                 : (!more || st->c.iters >= st->c.maxit) ? LSB_STATUS_MAXIT
                                                         : LSB_STATUS_RUNNING;
}

// alpha = rho/sigma ; s = r - alpha v (in place in r) ; s^ = D^-1 s (into the second gather vector) ;
// partials of s.s
template <bool V2>
__global__ __launch_bounds__(WG) void k_bcg_s(unsigned n, double *__restrict__ r, const double *__restrict__ v,
                                              const double *__restrict__ dinv, double dc,
                                              double *__restrict__ shat, lsb_bcg_state *__restrict__ st,
                                              int parity, const double *__restrict__ sig_parts, unsigned nsig,
                                              double *__restrict__ partials) {
  __shared__ double sred[4];
  BCG_IDX;
  const int stopped = st->c.status;
  const double rho = st->rho[parity];
  double sg[1];
  wg_sum_partials<1>(sig_parts, nsig, sg, sred);
  if (stopped)
    return;
  const double sigma = sg[0], alpha = rho / sigma;
  if (BCG_LEADER)
    st->nspmv = st->nspmv + 1; // v = Op p^ has run (nobody else touches the word in this launch)
  if (!(rho != 0.0) || !(sigma != 0.0) || !isfinite(rho) || !isfinite(sigma) ||
      !isfinite(alpha)) { // the same decision in every workgroup
    if (BCG_LEADER)
      st->c.status = LSB_STATUS_BREAKDOWN;
    return;
  }
  if (BCG_LEADER)
    st->alpha = alpha;
  double acc[1] = {0.0};
  if (V2) {
    const b2v *d2 = (const b2v *)dinv;
    for (size_t i = gtid; i < n2; i += gsz) {
      const b2v rv = ((const b2v *)r)[i], vv = ((const b2v *)v)[i], dv = ldd2(d2, i, dc);
      const b2v sv = {fma(-alpha, vv.x, rv.x), fma(-alpha, vv.y, rv.y)};
      ((b2v *)r)[i] = sv;
      ((b2v *)shat)[i] = b2v{dv.x * sv.x, dv.y * sv.y};
      acc[0] = fma(sv.y, sv.y, fma(sv.x, sv.x, acc[0]));
    }
  }
  for (size_t i = V2 ? (tail ? n - 1 : n) : gtid; i < n; i += gsz) {
    const double sv = fma(-alpha, v[i], r[i]);
    r[i] = sv;
    shat[i] = (dinv ? dinv[i] : dc) * sv;
    acc[0] = fma(sv, sv, acc[0]);
  }
  wg_sum<1>(acc, sred);
  if (threadIdx.x == 0)
    partials[blockIdx.x] = acc[0];
}

// partials of t.t
template <bool V2>
__global__ __launch_bounds__(WG) void k_bcg_tt(unsigned n, const double *__restrict__ t,
                                               const lsb_bcg_state *__restrict__ st,
                                               double *__restrict__ partials) {
  __shared__ double sred[4];
  BCG_IDX;
  if (st->c.status)
    return;
  double acc[1] = {0.0};
  if (V2)
    for (size_t i = gtid; i < n2; i += gsz) {
      const b2v tv = ((const b2v *)t)[i]; // (k_bcg_xr reads it next: the plain way)
      acc[0] = fma(tv.y, tv.y, fma(tv.x, tv.x, acc[0]));
    }
  for (size_t i = V2 ? (tail ? n - 1 : n) : gtid; i < n; i += gsz)
    acc[0] = fma(t[i], t[i], acc[0]);
  wg_sum<1>(acc, sred);
  if (threadIdx.x == 0)
    partials[blockIdx.x] = acc[0];
}

// the half step (ss <= tol^2 bb: x += alpha p^, r = s stands), or
// omega = ts/tt ; x += alpha p^ + omega s^ ; r = s - omega t (in place) ; partials of (r.r, r^.r)
template <bool V2>
__global__ __launch_bounds__(WG) void k_bcg_xr(unsigned n, double *__restrict__ x,
                                               const double *__restrict__ phat,
                                               const double *__restrict__ shat, double *__restrict__ r,
                                               const double *__restrict__ t,
                                               const double *__restrict__ rhat,
                                               lsb_bcg_state *__restrict__ st,
                                               const double *__restrict__ ss_parts, unsigned nss,
                                               const double *__restrict__ ts_parts, unsigned nts,
                                               const double *__restrict__ tt_parts, unsigned ntt,
                                               double *__restrict__ partials2) {
  __shared__ double sred[8];
  BCG_IDX;
  const int stopped = st->c.status;
  const double alpha = st->alpha, thresh2 = st->c.thresh2; // (alpha: k_bcg_s, two launches ago)
  double a[1], b[1], c[1];
  wg_sum_partials<1>(ss_parts, nss, a, sred);
  wg_sum_partials<1>(ts_parts, nts, b, sred);
  wg_sum_partials<1>(tt_parts, ntt, c, sred);
  if (stopped)
    return;
  const double ss = a[0], ts = b[0], tt = c[0];
  if (ss <= thresh2) {
    // every workgroup finishes its part of x before anybody may read CONVERGED: this launch
    // raises `half`, k_bcg_p behind it sets the status
    if (BCG_LEADER) {
      st->c.rr = ss;
      st->c.iters = st->c.iters + 1;
      st->half = 1;
    }
    if (V2)
      for (size_t i = gtid; i < n2; i += gsz) {
        b2v xv = ldnt((const b2v *)x + i);
        const b2v pv = ((const b2v *)phat)[i];
        xv.x = fma(alpha, pv.x, xv.x), xv.y = fma(alpha, pv.y, xv.y);
        ((b2v *)x)[i] = xv;
      }
    for (size_t i = V2 ? (tail ? n - 1 : n) : gtid; i < n; i += gsz)
      x[i] = fma(alpha, phat[i], x[i]);
    return;
  }
  const double omega = ts / tt;
  if (BCG_LEADER)
    st->nspmv = st->nspmv + 1; // t = Op s^ counts
  if (!(tt != 0.0) || !isfinite(tt) || !isfinite(ts) || !isfinite(omega)) {
    if (BCG_LEADER)
      st->c.status = LSB_STATUS_BREAKDOWN;
    return;
  }
  if (BCG_LEADER)
    st->omega = omega;
  double acc[2] = {0.0, 0.0};
  if (V2) {
    for (size_t i = gtid; i < n2; i += gsz) {
      b2v xv = ldnt((const b2v *)x + i);
      const b2v pv = ldnt((const b2v *)phat + i), hv = ldnt((const b2v *)shat + i);
      const b2v sv = ((const b2v *)r)[i], tv = ldnt((const b2v *)t + i), qv = ldnt((const b2v *)rhat + i);
      xv.x = fma(omega, hv.x, fma(alpha, pv.x, xv.x));
      xv.y = fma(omega, hv.y, fma(alpha, pv.y, xv.y));
      const b2v rv = {fma(-omega, tv.x, sv.x), fma(-omega, tv.y, sv.y)};
      __builtin_nontemporal_store(xv, (b2v *)x + i); // nobody reads x before the next iteration
      ((b2v *)r)[i] = rv;
      acc[0] = fma(rv.y, rv.y, fma(rv.x, rv.x, acc[0]));
      acc[1] = fma(qv.y, rv.y, fma(qv.x, rv.x, acc[1]));
    }
  }
  for (size_t i = V2 ? (tail ? n - 1 : n) : gtid; i < n; i += gsz) {
    x[i] = fma(omega, shat[i], fma(alpha, phat[i], x[i]));
    const double rv = fma(-omega, t[i], r[i]);
    r[i] = rv;
    acc[0] = fma(rv, rv, acc[0]);
    acc[1] = fma(rhat[i], rv, acc[1]);
  }
  wg_sum<2>(acc, sred);
  if (threadIdx.x == 0) {
    partials2[2 * blockIdx.x + 0] = acc[0];
    partials2[2 * blockIdx.x + 1] = acc[1];
  }
}

// (rr, rho') = sum partials ; stop test ; beta = (rho'/rho)(alpha/omega) ;
// p = r + beta (p - omega v) ; p^ = D^-1 p (into the gather vector)
template <bool V2>
__global__ __launch_bounds__(WG) void k_bcg_p(unsigned n, const double *__restrict__ r, double *__restrict__ p,
                                              const double *__restrict__ v, const double *__restrict__ dinv,
                                              double dc, double *__restrict__ phat,
                                              lsb_bcg_state *__restrict__ st, int parity,
                                              const double *__restrict__ parts2, unsigned nparts2) {
  __shared__ double sred[8];
  BCG_IDX;
  const int stopped = st->c.status, half = st->half;
  const double rho_old = st->rho[parity], alpha = st->alpha, omega = st->omega, thresh2 = st->c.thresh2;
  double s2[2];
  wg_sum_partials<2>(parts2, nparts2, s2, sred);
  if (stopped)
    return;
  if (half) { // k_bcg_xr took the half step (and counted the iteration)
    if (BCG_LEADER)
      st->c.status = LSB_STATUS_CONVERGED;
    return;
  }
  const double rr = s2[0], rho_new = s2[1];
  const bool conv = rr <= thresh2;
  if (BCG_LEADER) { // only this thread touches iters / rr / rho[parity ^ 1] / status in this launch
    const int it = st->c.iters + 1;
    st->c.iters = it;
    st->c.rr = rr;
    st->rho[parity ^ 1] = rho_new;
    if (conv)
      st->c.status = LSB_STATUS_CONVERGED;
    else if (!(omega != 0.0))
      st->c.status = LSB_STATUS_BREAKDOWN;
    else if (it >= st->c.maxit)
      st->c.status = LSB_STATUS_MAXIT;
  }
  if (conv || !(omega != 0.0))
    return;
  const double beta = (rho_new / rho_old) * (alpha / omega);
  if (V2) {
    const b2v *d2 = (const b2v *)dinv;
    for (size_t i = gtid; i < n2; i += gsz) {
      const b2v rv = ((const b2v *)r)[i], vv = ldnt((const b2v *)v + i), dv = ldd2(d2, i, dc);
      b2v pv = ((const b2v *)p)[i];
      pv.x = fma(beta, fma(-omega, vv.x, pv.x), rv.x);
      pv.y = fma(beta, fma(-omega, vv.y, pv.y), rv.y);
      ((b2v *)p)[i] = pv;
      ((b2v *)phat)[i] = b2v{dv.x * pv.x, dv.y * pv.y}; // the SpMV gathers it next: the plain way
    }
  }
  for (size_t i = V2 ? (tail ? n - 1 : n) : gtid; i < n; i += gsz) {
    const double pv = fma(beta, fma(-omega, v[i], p[i]), r[i]);
    p[i] = pv;
    phat[i] = (dinv ? dinv[i] : dc) * pv;
  }
}

extern "C" {

void lsb_k_bcg_init(unsigned n, const double *b, const double *dinv, double dc, double *x, double *r,
                    double *rhat, double *p, double *phat, double *partials, unsigned *npartials,
                    void *stream) {
  const unsigned g = lsb_k_blas1_grid(n);
  *npartials = g;
  const bool v2 = aligned16(b) && aligned16(dinv) && aligned16(x) && aligned16(r) && aligned16(rhat) &&
                  aligned16(p) && aligned16(phat);
  const auto kern = v2 ? k_bcg_init<true> : k_bcg_init<false>;
  kern<<<g, WG, 0, (hipStream_t)stream>>>(n, b, dinv, dc, x, r, rhat, p, phat, partials);
}

void lsb_k_bcg_init_state(struct lsb_bcg_state *st, const double *parts, unsigned nparts, double tol,
                          int maxit, void *stream) {
  k_bcg_init_state<<<1, WG, 0, (hipStream_t)stream>>>(st, parts, nparts, tol, maxit);
}

void lsb_k_bcg_restart(unsigned n, const double *b, const double *ax, const double *dinv, double dc,
                       double *r, double *rhat, double *p, double *phat, double *partials,
                       unsigned *npartials, void *stream) {
  const unsigned g = lsb_k_blas1_grid(n);
  *npartials = g;
  const bool v2 = aligned16(b) && aligned16(ax) && aligned16(dinv) && aligned16(r) && aligned16(rhat) &&
                  aligned16(p) && aligned16(phat);
  const auto kern = v2 ? k_bcg_restart<true> : k_bcg_restart<false>;
  kern<<<g, WG, 0, (hipStream_t)stream>>>(n, b, ax, dinv, dc, r, rhat, p, phat, partials);
}

void lsb_k_bcg_restart_state(struct lsb_bcg_state *st, const double *parts, unsigned nparts, int more,
                             void *stream) {
  k_bcg_restart_state<<<1, WG, 0, (hipStream_t)stream>>>(st, parts, nparts, more);
}

void lsb_k_bcg_s(unsigned n, double *r, const double *v, const double *dinv, double dc, double *shat,
                 struct lsb_bcg_state *st, int parity, const double *sig_parts, unsigned nsig,
                 double *partials, unsigned *npartials, void *stream) {
  const unsigned g = lsb_k_blas1_grid(n);
  *npartials = g;
  const bool v2 = aligned16(r) && aligned16(v) && aligned16(dinv) && aligned16(shat);
  const auto kern = v2 ? k_bcg_s<true> : k_bcg_s<false>;
  kern<<<g, WG, 0, (hipStream_t)stream>>>(n, r, v, dinv, dc, shat, st, parity, sig_parts, nsig, partials);
}

void lsb_k_bcg_tt(unsigned n, const double *t, const struct lsb_bcg_state *st, double *partials,
                  unsigned *npartials, void *stream) {
  const unsigned g = lsb_k_blas1_grid(n);
  *npartials = g;
  const auto kern = aligned16(t) ? k_bcg_tt<true> : k_bcg_tt<false>;
  kern<<<g, WG, 0, (hipStream_t)stream>>>(n, t, st, partials);
}

void lsb_k_bcg_xr(unsigned n, double *x, const double *phat, const double *shat, double *r, const double *t,
                  const double *rhat, struct lsb_bcg_state *st, const double *ss_parts, unsigned nss,
                  const double *ts_parts, unsigned nts, const double *tt_parts, unsigned ntt,
                  double *partials2, unsigned *npartials, void *stream) {
  const unsigned g = lsb_k_blas1_grid(n);
  *npartials = g;
  const bool v2 = aligned16(x) && aligned16(phat) && aligned16(shat) && aligned16(r) && aligned16(t) &&
                  aligned16(rhat);
  const auto kern = v2 ? k_bcg_xr<true> : k_bcg_xr<false>;
  kern<<<g, WG, 0, (hipStream_t)stream>>>(n, x, phat, shat, r, t, rhat, st, ss_parts, nss, ts_parts, nts,
                                          tt_parts, ntt, partials2);
}

void lsb_k_bcg_p(unsigned n, const double *r, double *p, const double *v, const double *dinv, double dc,
                 double *phat, struct lsb_bcg_state *st, int parity, const double *parts2, unsigned nparts2,
                 void *stream) {
  const unsigned g = lsb_k_blas1_grid(n);
  const bool v2 = aligned16(r) && aligned16(p) && aligned16(v) && aligned16(dinv) && aligned16(phat);
  const auto kern = v2 ? k_bcg_p<true> : k_bcg_p<false>;
  kern<<<g, WG, 0, (hipStream_t)stream>>>(n, r, p, v, dinv, dc, phat, st, parity, parts2, nparts2);
}

} // extern "C"
