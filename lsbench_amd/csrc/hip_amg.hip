// Smoothed-aggregation AMG V-cycle (LSB_PRECOND_AMG): z = M^-1 r as one symmetric V-cycle from a
// zero initial guess, l1-Jacobi smoothing (M_l = diag(sum_j |a_ij|): convergent for every SPD
// level, so the cycle is SPD and safe inside CG).  On level l, with nu = opts.amg_sweeps:
//     x = M^-1 b;  (nu - 1) x  x += M^-1 (b - A x)
//     r = b - A x;  b_c = R r;  recurse (the coarsest level: x_c = coarse_inv b_c)
//     x += P x_c;  nu x  x += M^-1 (b - A x)
// The hierarchy is built on the host at solver creation (lsb_amg.c); hip_amg_drv.c uploads it and
// enqueues the launches below.  Everything here is a row kernel over a CSR:
//
// k_amg_csr<L, MODE>  L lanes per row (a sub-wavefront of the wave64, per level and per matrix from
//                     the mean row length: coarse operators have much longer rows than the fine one);
//                     MODE sweep (out of place, ping-pong buffers), residual, rectangular SpMV (the
//                     restriction), or x += P e in place (row i reads only x_i of x).
// k_amg_tail          ONE workgroup of 1024 threads runs every level of at most opts.amg_tail_rows
//                     rows and the dense coarse solve in one launch, steps separated by
//                     __syncthreads(); the level vectors stay in L2.  Meant to save the 1.2-1.9 us
//                     boundary of each small step; measured slower at every size (one workgroup
//                     walks a level's rows in passes of dependent L2 loads), so it is off by
//                     default (opts.amg_tail_rows = 0; profiles/r05_amg.txt).
//
// k_amg_cheb<L>      opts.amg_smoother = LSB_AMG_SMOOTH_CHEB: one step of the Chebyshev polynomial of degree nu
//                     in D^-1 A in the place of a sweep -- the same row product, then
//                         d_i <- fma(c2 / a_ii, b_i - s_i, c1 d_i),  y_i = x_i + d_i
//                     (d in place: row i reads only d_i; c1 == 0 on step 0, which does not read d).  The
//                     coefficients come from the host in fp64 (lsb_amg_cheb_coeffs) on the interval
//                     [rho / ratio, rho], rho the level's Gershgorin bound.  k_amg_cheb_first is step 0 from
//                     the zero guess: d = (c2 / a_ii) b, x = d, no matrix.  The cycle has the launches and
//                     the ping-pong parity of the l1-Jacobi one; the one-launch tail is not built for it.
//
// No atomics: every output row is one lane group's fixed-order reduction (amg_row), the same
// function in both kernels, so z is bitwise repeatable and the tail on and off give the same bits.
// Every kernel is a no-op once the solve's state has left RUNNING.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hip_amg_cheb.h"
#include "hip_kcommon.h"

#define AMG_WG 256
#define AMG_TAIL 1024

// a row of the CSR times x: lane `lane` of L takes entries lane, lane + L, ... in storage order, then
// a butterfly over the L lanes (a + b == b + a: every lane ends with the same bits)
template <int L>
__device__ __forceinline__ double amg_row(const int *offs, const int *cols, const double *vals, const double *x,
                                          unsigned i, unsigned lane) {
  double acc = 0.0;
  const int e1 = offs[i + 1];
  for (int e = offs[i] + (int)lane; e < e1; e += L)
    acc = fma(vals[e], x[cols[e]], acc);
#pragma unroll
  for (int o = L / 2; o > 0; o >>= 1)
    acc += __shfl_xor(acc, o, L);
  return acc;
}

// a row of the dense nc x nc coarse inverse times b, the same order
template <int L>
__device__ __forceinline__ double amg_dense_row(const double *c, unsigned nc, const double *b, unsigned i,
                                                unsigned lane) {
  double acc = 0.0;
  const double *ci = c + (size_t)i * nc;
  for (unsigned j = lane; j < nc; j += L)
    acc = fma(ci[j], b[j], acc);
#pragma unroll
  for (int o = L / 2; o > 0; o >>= 1)
    acc += __shfl_xor(acc, o, L);
  return acc;
}

// what lane 0 of row i's group writes, given s = (row of the matrix) . xin
template <int MODE>
__device__ __forceinline__ void amg_finish(unsigned i, double s, const double *xin, const double *b,
                                           const double *minv, double *y) {
  if (MODE == LSB_AMG_SWEEP)
    y[i] = fma(minv[i], b[i] - s, xin[i]);
  else if (MODE == LSB_AMG_RESID)
    y[i] = b[i] - s;
  else if (MODE == LSB_AMG_SPMV)
    y[i] = s;
  else
    y[i] = y[i] + s;
}

template <int L, int MODE>
__global__ __launch_bounds__(AMG_WG) void k_amg_csr(unsigned n, const int *__restrict__ offs,
                                                    const int *__restrict__ cols, const double *__restrict__ vals,
                                                    const double *xin, const double *b, const double *minv, double *y,
                                                    const struct lsb_pcg_state *st) {
  if (st && st->status)
    return;
  const unsigned long long stride = (unsigned long long)gridDim.x * AMG_WG; // a multiple of L: groups stay whole
  for (unsigned long long g = (unsigned long long)blockIdx.x * AMG_WG + threadIdx.x; g / L < n; g += stride) {
    const unsigned i = (unsigned)(g / L), lane = (unsigned)(g % L);
    const double s = amg_row<L>(offs, cols, vals, xin, i, lane);
    if (lane == 0)
      amg_finish<MODE>(i, s, xin, b, minv, y);
  }
}

__global__ __launch_bounds__(AMG_WG) void k_amg_first(unsigned n, const double *__restrict__ b,
                                                      const double *__restrict__ minv, double *__restrict__ x,
                                                      const struct lsb_pcg_state *st) {
  if (st && st->status)
    return;
  for (unsigned i = blockIdx.x * AMG_WG + threadIdx.x; i < n; i += gridDim.x * AMG_WG)
    x[i] = minv[i] * b[i];
}

// one Chebyshev step: y = xin + d', d' = c1 d + c2 D^-1 (b - A xin), d updated in place
template <int L>
__global__ __launch_bounds__(AMG_WG) void k_amg_cheb(unsigned n, const int *__restrict__ offs,
                                                     const int *__restrict__ cols, const double *__restrict__ vals,
                                                     const double *xin, const double *b, const double *dinv, double c1,
                                                     double c2, double *d, double *y, const struct lsb_pcg_state *st) {
  if (st && st->status)
    return;
  const unsigned long long stride = (unsigned long long)gridDim.x * AMG_WG; // a multiple of L: groups stay whole
  for (unsigned long long g = (unsigned long long)blockIdx.x * AMG_WG + threadIdx.x; g / L < n; g += stride) {
    const unsigned i = (unsigned)(g / L), lane = (unsigned)(g % L);
    const double s = amg_row<L>(offs, cols, vals, xin, i, lane);
    if (lane == 0) {
      const double dn = amg_cheb_dir(c1, c2, dinv[i], b[i], s, c1 != 0.0 ? d[i] : 0.0);
      d[i] = dn;
      y[i] = xin[i] + dn;
    }
  }
}

// step 0 from the zero guess: d = (c2 D^-1) b, x = d
__global__ __launch_bounds__(AMG_WG) void k_amg_cheb_first(unsigned n, const double *__restrict__ b,
                                                           const double *__restrict__ dinv, double c2,
                                                           double *__restrict__ d, double *__restrict__ x,
                                                           const struct lsb_pcg_state *st) {
  if (st && st->status)
    return;
  for (unsigned i = blockIdx.x * AMG_WG + threadIdx.x; i < n; i += gridDim.x * AMG_WG) {
    const double v = amg_cheb_dir(0.0, c2, dinv[i], b[i], 0.0, 0.0);
    d[i] = v;
    x[i] = v;
  }
}

template <int L>
__global__ __launch_bounds__(AMG_WG) void k_amg_dense(unsigned nc, const double *__restrict__ c,
                                                      const double *__restrict__ b, double *__restrict__ out,
                                                      const struct lsb_pcg_state *st) {
  if (st && st->status)
    return;
  for (unsigned g = blockIdx.x * AMG_WG + threadIdx.x; g / L < nc; g += gridDim.x * AMG_WG) {
    const unsigned i = g / L, lane = g % L;
    const double s = amg_dense_row<L>(c, nc, b, i, lane);
    if (lane == 0)
      out[i] = s;
  }
}

// ---- the one-launch tail ------------------------------------------------------------------------
// every pass walks its rows in groups of L threads (1024 / L rows at a time) and ends in a barrier
template <int L, int MODE>
__device__ __forceinline__ void tail_rows(const struct lsb_amg_mat &m, const double *xin, const double *b,
                                          const double *minv, double *y) {
  const unsigned lane = threadIdx.x % L;
  for (unsigned i = threadIdx.x / L; i < m.rows; i += AMG_TAIL / L) {
    const double s = amg_row<L>(m.offs, m.cols, m.vals, xin, i, lane);
    if (lane == 0)
      amg_finish<MODE>(i, s, xin, b, minv, y);
  }
}

template <int MODE>
__device__ void tail_pass(const struct lsb_amg_mat &m, const double *xin, const double *b, const double *minv,
                          double *y) {
  switch (m.lanes) {
  case 2: tail_rows<2, MODE>(m, xin, b, minv, y); break;
  case 4: tail_rows<4, MODE>(m, xin, b, minv, y); break;
  case 8: tail_rows<8, MODE>(m, xin, b, minv, y); break;
  case 16: tail_rows<16, MODE>(m, xin, b, minv, y); break;
  case 32: tail_rows<32, MODE>(m, xin, b, minv, y); break;
  default: tail_rows<64, MODE>(m, xin, b, minv, y); break;
  }
  __syncthreads();
}

template <int L>
__device__ __forceinline__ void tail_dense_rows(const double *c, unsigned nc, const double *b, double *out) {
  const unsigned lane = threadIdx.x % L;
  for (unsigned i = threadIdx.x / L; i < nc; i += AMG_TAIL / L) {
    const double s = amg_dense_row<L>(c, nc, b, i, lane);
    if (lane == 0)
      out[i] = s;
  }
}

__global__ __launch_bounds__(AMG_TAIL) void k_amg_tail(const struct lsb_amg_lvdev *lv, unsigned t, unsigned nlev,
                                                       unsigned nu, const double *cinv, unsigned nc,
                                                       unsigned clanes, const double *b0, double *out0,
                                                       const struct lsb_pcg_state *st) {
  if (st && st->status)
    return;
  // down: pre-smoothing, residual, restriction
  for (unsigned l = t; l + 1 < nlev; l++) {
    const struct lsb_amg_lvdev &v = lv[l];
    const double *b = l ? v.b : b0;
    double *out = l ? v.out : out0;
    for (unsigned i = threadIdx.x; i < v.n; i += AMG_TAIL)
      v.tmp[i] = v.minv[i] * b[i];
    __syncthreads();
    double *cur = v.tmp, *oth = out;
    for (unsigned k = 1; k < nu; k++) {
      tail_pass<LSB_AMG_SWEEP>(v.A, cur, b, v.minv, oth);
      double *w = cur;
      cur = oth, oth = w;
    }
    tail_pass<LSB_AMG_RESID>(v.A, cur, b, v.minv, v.r);
    tail_pass<LSB_AMG_SPMV>(v.R, v.r, nullptr, nullptr, lv[l + 1].b);
  }
  {
    const unsigned c = nlev - 1;
    const double *b = c ? lv[c].b : b0;
    double *out = c ? lv[c].out : out0;
    switch (clanes) {
    case 2: tail_dense_rows<2>(cinv, nc, b, out); break;
    case 4: tail_dense_rows<4>(cinv, nc, b, out); break;
    case 8: tail_dense_rows<8>(cinv, nc, b, out); break;
    case 16: tail_dense_rows<16>(cinv, nc, b, out); break;
    case 32: tail_dense_rows<32>(cinv, nc, b, out); break;
    default: tail_dense_rows<64>(cinv, nc, b, out); break;
    }
    __syncthreads();
  }
  // up: prolongation, post-smoothing; 2 nu - 1 out-of-place sweeps in all end in `out`
  for (unsigned l = nlev - 1; l-- > t;) {
    const struct lsb_amg_lvdev &v = lv[l];
    const double *b = l ? v.b : b0;
    double *out = l ? v.out : out0;
    double *cur = (nu - 1) % 2 ? out : v.tmp, *oth = (nu - 1) % 2 ? v.tmp : out;
    tail_pass<LSB_AMG_ADDP>(v.P, lv[l + 1].out, nullptr, nullptr, cur);
    for (unsigned k = 0; k < nu; k++) {
      tail_pass<LSB_AMG_SWEEP>(v.A, cur, b, v.minv, oth);
      double *w = cur;
      cur = oth, oth = w;
    }
  }
}

extern "C" {

static unsigned amg_grid(unsigned long long threads) {
  const unsigned long long g = (threads + AMG_WG - 1) / AMG_WG;
  return g > 16384ull ? 16384u : (g ? (unsigned)g : 1u);
}

void lsb_k_amg_first(unsigned n, const double *b, const double *minv, double *x, const struct lsb_pcg_state *st,
                     void *stream) {
  if (n)
    k_amg_first<<<amg_grid(n), AMG_WG, 0, (hipStream_t)stream>>>(n, b, minv, x, st);
}

void lsb_k_amg_csr(int mode, const struct lsb_amg_mat *m, const double *xin, const double *b, const double *minv,
                   double *y, const struct lsb_pcg_state *st, void *stream) {
  if (!m->rows)
    return;
  hipStream_t s = (hipStream_t)stream;
  const unsigned g = amg_grid((unsigned long long)m->rows * m->lanes);
#define AMG_MODE(MM)                                                                                            \
  case MM:                                                                                                      \
    LANES_DISPATCH(m->lanes, (k_amg_csr<L, MM><<<g, AMG_WG, 0, s>>>(m->rows, m->offs, m->cols, m->vals, xin, b, \
                                                                    minv, y, st)));                             \
    break;
  switch (mode) {
    AMG_MODE(LSB_AMG_SWEEP) AMG_MODE(LSB_AMG_RESID) AMG_MODE(LSB_AMG_SPMV) AMG_MODE(LSB_AMG_ADDP)
  default:
    errx(EXIT_FAILURE, "lsb_k_amg_csr: no mode %d", mode);
  }
#undef AMG_MODE
}

void lsb_k_amg_cheb_first(unsigned n, const double *b, const double *dinv, double c2, double *d, double *x,
                          const struct lsb_pcg_state *st, void *stream) {
  if (n)
    k_amg_cheb_first<<<amg_grid(n), AMG_WG, 0, (hipStream_t)stream>>>(n, b, dinv, c2, d, x, st);
}

void lsb_k_amg_cheb(const struct lsb_amg_mat *m, const double *xin, const double *b, const double *dinv, double c1,
                    double c2, double *d, double *y, const struct lsb_pcg_state *st, void *stream) {
  if (!m->rows)
    return;
  hipStream_t s = (hipStream_t)stream;
  const unsigned g = amg_grid((unsigned long long)m->rows * m->lanes);
  LANES_DISPATCH(m->lanes, (k_amg_cheb<L><<<g, AMG_WG, 0, s>>>(m->rows, m->offs, m->cols, m->vals, xin, b, dinv, c1, c2,
                                                               d, y, st)));
}

void lsb_k_amg_dense(unsigned nc, unsigned lanes, const double *cinv, const double *b, double *out,
                     const struct lsb_pcg_state *st, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  const unsigned g = amg_grid((unsigned long long)nc * lanes);
  LANES_DISPATCH(lanes, (k_amg_dense<L><<<g, AMG_WG, 0, s>>>(nc, cinv, b, out, st)));
}

void lsb_k_amg_tail(const struct lsb_amg_lvdev *lv, unsigned t, unsigned nlev, unsigned nu, const double *cinv,
                    unsigned nc, unsigned clanes, const double *b0, double *out0, const struct lsb_pcg_state *st,
                    void *stream) {
  k_amg_tail<<<1, AMG_TAIL, 0, (hipStream_t)stream>>>(lv, t, nlev, nu, cinv, nc, clanes, b0, out0, st);
}

} // extern "C"
