// The AMG V-cycle in fp32 (opts.amg_precision = LSB_AMG_PREC_FP32, --amg-precision fp32): hip_amg.hip's cycle --
// the same steps, launch count, lane rule and ping-pong parity (driver: amg_cycle in hip_amg_drv.c) -- on a
// hierarchy held in single precision, inside a Krylov loop that stays in fp64.  The cycle is bandwidth-bound and
// only has to be a good approximate inverse, so it moves 8 B per stored entry and 4 B per vector element where
// the fp64 cycle moves 12 B and 8 B.
//
// Layout: a matrix (A_l, P_l, R_l) is its int row offsets plus ONE 8-byte word per stored entry, the 0-based
// column in the low 32 bits and the bits of (float)value in the high 32 (lsb_csr_pack_f32): one 8-byte load
// where the fp64 kernels issue a 4-byte and an 8-byte one.  minv (l1-Jacobi) or dinv (Chebyshev), the coarse
// inverse, every level vector and the Chebyshev direction d are float.
//
// Rounding rule, the same in every kernel of this file:
//   1. lane l of a row's L lanes takes the entries l, l + L, ... in storage order: a = fmaf(val_j, x[col_j], a);
//   2. the L lane sums are folded by the xor butterfly L/2, ..., 1 with float additions (a + b == b + a: every
//      lane ends with the same bits);
//   3. lane 0 finishes in float --  SWEEP: fmaf(minv_i, b_i - s, x_i);  RESID: b_i - s;  SPMV: s;  ADDP: y_i + s;
//      Chebyshev direction: fmaf(c2 dinv_i, b_i - s, c1 d_i), and (c2 dinv_i) (b_i - s) where c1 == 0 (d is not read).
// Nothing is in double except the two ends: IN64 kernels (the fine level's first step; the coarse solve of a
// one-level hierarchy) read the caller's fp64 r and round it ONCE to float -- the first step also stores that
// copy, which every later step of the level reads -- and OUT64 kernels (the fine level's last post-smoothing
// launch; that coarse solve) store their float result widened to double, which is exact, straight into z.  There
// is no conversion launch at either end.  The Chebyshev coefficients are computed by the host in fp64 at set-up and
// rounded to float where they are passed as kernel arguments (a captured graph keeps them).
//
// Range: r is rounded to float UNSCALED.  Components beyond +-3.4e38 overflow to infinity and components below
// about 1e-38 lose bits (subnormal) -- with b_i = i and tol 1e-12 the residual stays some 30 orders of magnitude
// away from either end.  Set-up refuses a hierarchy one of whose entries does not fit a float.
//
// No atomics, no allocation, no synchronisation inside an application: every output row is one lane group's
// fixed-order reduction, so z is bitwise repeatable.  Every kernel is a no-op once the solve's state has left
// RUNNING.  Blocks of columns: hip_amg_f32_m.hip (l1-Jacobi; each column with this file's bits).  Not built: the
// one-launch tail.
#include "hip_kcommon.h"

#define AMG32_WG 256

typedef unsigned long long amg32_ent; // {col : 32 low, float bits : 32 high}

template <int L>
__device__ __forceinline__ float amg32_fold(float acc) {
#pragma unroll
  for (int o = L / 2; o > 0; o >>= 1)
    acc += __shfl_xor(acc, o, L);
  return acc;
}

// a row of the packed CSR times x (rules 1 and 2)
template <int L>
__device__ __forceinline__ float amg32_row(const int *offs, const amg32_ent *ent, const float *x, unsigned i,
                                           unsigned lane) {
  float acc = 0.0f;
  const int e1 = offs[i + 1];
  for (int e = offs[i] + (int)lane; e < e1; e += L) {
    const amg32_ent w = ent[e];
    acc = fmaf(__uint_as_float((unsigned)(w >> 32)), x[(unsigned)w], acc);
  }
  return amg32_fold<L>(acc);
}

template <bool IN64>
__device__ __forceinline__ float amg32_in(const void *b, size_t i) {
  return IN64 ? (float)((const double *)b)[i] : ((const float *)b)[i];
}

// the Chebyshev direction of a row (rule 3); d is not looked at where c1 == 0
__device__ __forceinline__ float amg32_cheb_dir(float c1, float c2, float dinv, float b, float s, float d) {
  const float m = c2 * dinv, t = b - s;
  return c1 == 0.0f ? m * t : fmaf(m, t, c1 * d);
}

// y64 (OUT64) takes the result in the place of y
template <int L, int MODE, bool OUT64>
__global__ __launch_bounds__(AMG32_WG) void k_amg32_csr(unsigned n, const int *__restrict__ offs,
                                                        const amg32_ent *__restrict__ ent, const float *xin,
                                                        const float *b, const float *minv, float *y, double *y64,
                                                        const struct lsb_pcg_state *st) {
  if (st && st->status)
    return;
  const unsigned long long stride = (unsigned long long)gridDim.x * AMG32_WG; // a multiple of L: groups stay whole
  for (unsigned long long g = (unsigned long long)blockIdx.x * AMG32_WG + threadIdx.x; g / L < n; g += stride) {
    const unsigned i = (unsigned)(g / L), lane = (unsigned)(g % L);
    const float s = amg32_row<L>(offs, ent, xin, i, lane);
    if (lane == 0) {
      float v;
      if (MODE == LSB_AMG_SWEEP)
        v = fmaf(minv[i], b[i] - s, xin[i]);
      else if (MODE == LSB_AMG_RESID)
        v = b[i] - s;
      else if (MODE == LSB_AMG_SPMV)
        v = s;
      else
        v = y[i] + s;
      if (OUT64)
        y64[i] = (double)v;
      else
        y[i] = v;
    }
  }
}

// x = minv b from the zero guess; IN64: b is the caller's fp64 r, rounded once, the copy kept in b32
template <bool IN64>
__global__ __launch_bounds__(AMG32_WG) void k_amg32_first(unsigned n, const void *__restrict__ b,
                                                          const float *__restrict__ minv, float *__restrict__ x,
                                                          float *__restrict__ b32, const struct lsb_pcg_state *st) {
  if (st && st->status)
    return;
  for (unsigned i = blockIdx.x * AMG32_WG + threadIdx.x; i < n; i += gridDim.x * AMG32_WG) {
    const float bi = amg32_in<IN64>(b, i);
    if (IN64)
      b32[i] = bi;
    x[i] = minv[i] * bi;
  }
}

// one Chebyshev step: y = xin + d', d' = c1 d + c2 D^-1 (b - A xin), d updated in place
template <int L, bool OUT64>
__global__ __launch_bounds__(AMG32_WG) void k_amg32_cheb(unsigned n, const int *__restrict__ offs,
                                                         const amg32_ent *__restrict__ ent, const float *xin,
                                                         const float *b, const float *dinv, float c1, float c2,
                                                         float *d, float *y, double *y64,
                                                         const struct lsb_pcg_state *st) {
  if (st && st->status)
    return;
  const unsigned long long stride = (unsigned long long)gridDim.x * AMG32_WG;
  for (unsigned long long g = (unsigned long long)blockIdx.x * AMG32_WG + threadIdx.x; g / L < n; g += stride) {
    const unsigned i = (unsigned)(g / L), lane = (unsigned)(g % L);
    const float s = amg32_row<L>(offs, ent, xin, i, lane);
    if (lane == 0) {
      const float dn = amg32_cheb_dir(c1, c2, dinv[i], b[i], s, c1 != 0.0f ? d[i] : 0.0f);
      d[i] = dn;
      const float v = xin[i] + dn;
      if (OUT64)
        y64[i] = (double)v;
      else
        y[i] = v;
    }
  }
}

// step 0 from the zero guess: d = (c2 D^-1) b, x = d; IN64 as k_amg32_first
template <bool IN64>
__global__ __launch_bounds__(AMG32_WG) void k_amg32_cheb_first(unsigned n, const void *__restrict__ b,
                                                               const float *__restrict__ dinv, float c2,
                                                               float *__restrict__ d, float *__restrict__ x,
                                                               float *__restrict__ b32,
                                                               const struct lsb_pcg_state *st) {
  if (st && st->status)
    return;
  for (unsigned i = blockIdx.x * AMG32_WG + threadIdx.x; i < n; i += gridDim.x * AMG32_WG) {
    const float bi = amg32_in<IN64>(b, i);
    if (IN64)
      b32[i] = bi;
    const float v = amg32_cheb_dir(0.0f, c2, dinv[i], bi, 0.0f, 0.0f);
    d[i] = v;
    x[i] = v;
  }
}

// the coarse solve: a row of the dense nc x nc inverse times b, rules 1 and 2; IN64 / OUT64: a hierarchy of one
// level, from r to z
template <int L, bool IN64, bool OUT64>
__global__ __launch_bounds__(AMG32_WG) void k_amg32_dense(unsigned nc, const float *__restrict__ c,
                                                          const void *__restrict__ b, void *__restrict__ out,
                                                          const struct lsb_pcg_state *st) {
  if (st && st->status)
    return;
  for (unsigned g = blockIdx.x * AMG32_WG + threadIdx.x; g / L < nc; g += gridDim.x * AMG32_WG) {
    const unsigned i = g / L, lane = g % L;
    const float *ci = c + (size_t)i * nc;
    float acc = 0.0f;
    for (unsigned j = lane; j < nc; j += L)
      acc = fmaf(ci[j], amg32_in<IN64>(b, j), acc);
    acc = amg32_fold<L>(acc);
    if (lane == 0) {
      if (OUT64)
        ((double *)out)[i] = (double)acc;
      else
        ((float *)out)[i] = acc;
    }
  }
}

// --------------------------------------------------------------------------
// Launchers (C ABI; declared in lsb_impl.h).  lanes: 2 .. 64, a power of two.
// --------------------------------------------------------------------------
static unsigned amg32_grid(unsigned long long threads) {
  const unsigned long long g = (threads + AMG32_WG - 1) / AMG32_WG;
  return g > 16384ull ? 16384u : (g ? (unsigned)g : 1u);
}

extern "C" {

void lsb_k_amg32_first(unsigned n, int in64, const void *b, const float *minv, float *x, float *b32,
                       const struct lsb_pcg_state *st, void *stream) {
  if (!n)
    return;
  hipStream_t s = (hipStream_t)stream;
  if (in64)
    k_amg32_first<true><<<amg32_grid(n), AMG32_WG, 0, s>>>(n, b, minv, x, b32, st);
  else
    k_amg32_first<false><<<amg32_grid(n), AMG32_WG, 0, s>>>(n, b, minv, x, b32, st);
}

void lsb_k_amg32_csr(int mode, const struct amg_mat32 *m, const float *xin, const float *b, const float *minv,
                     float *y, double *y64, const struct lsb_pcg_state *st, void *stream) {
  if (!m->rows)
    return;
  hipStream_t s = (hipStream_t)stream;
  const unsigned g = amg32_grid((unsigned long long)m->rows * m->lanes);
  if (y64 && mode != LSB_AMG_SWEEP)
    errx(EXIT_FAILURE, "lsb_k_amg32_csr: only a sweep writes fp64");
#define AMG32_GO(MM, O64) LANES_DISPATCH(m->lanes, (k_amg32_csr<L, MM, O64><<<g, AMG32_WG, 0, s>>>(m->rows, m->offs, m->ent, xin, b, minv, y, y64, st)));
  switch (mode) {
  case LSB_AMG_SWEEP:
    if (y64)
      AMG32_GO(LSB_AMG_SWEEP, true)
    else
      AMG32_GO(LSB_AMG_SWEEP, false)
    break;
  case LSB_AMG_RESID: AMG32_GO(LSB_AMG_RESID, false) break;
  case LSB_AMG_SPMV: AMG32_GO(LSB_AMG_SPMV, false) break;
  case LSB_AMG_ADDP: AMG32_GO(LSB_AMG_ADDP, false) break;
  default: errx(EXIT_FAILURE, "lsb_k_amg32_csr: no mode %d", mode);
  }
#undef AMG32_GO
}

void lsb_k_amg32_cheb_first(unsigned n, int in64, const void *b, const float *dinv, float c2, float *d, float *x,
                            float *b32, const struct lsb_pcg_state *st, void *stream) {
  if (!n)
    return;
  hipStream_t s = (hipStream_t)stream;
  if (in64)
    k_amg32_cheb_first<true><<<amg32_grid(n), AMG32_WG, 0, s>>>(n, b, dinv, c2, d, x, b32, st);
  else
    k_amg32_cheb_first<false><<<amg32_grid(n), AMG32_WG, 0, s>>>(n, b, dinv, c2, d, x, b32, st);
}

void lsb_k_amg32_cheb(const struct amg_mat32 *m, const float *xin, const float *b, const float *dinv, float c1,
                      float c2, float *d, float *y, double *y64, const struct lsb_pcg_state *st, void *stream) {
  if (!m->rows)
    return;
  hipStream_t s = (hipStream_t)stream;
  const unsigned g = amg32_grid((unsigned long long)m->rows * m->lanes);
  if (y64)
    LANES_DISPATCH(m->lanes, (k_amg32_cheb<L, true><<<g, AMG32_WG, 0, s>>>(m->rows, m->offs, m->ent, xin, b, dinv, c1, c2, d, y, y64, st)));
  else
    LANES_DISPATCH(m->lanes, (k_amg32_cheb<L, false><<<g, AMG32_WG, 0, s>>>(m->rows, m->offs, m->ent, xin, b, dinv, c1, c2, d, y, y64, st)));
}

// ends64: a hierarchy of one level -- b is the caller's fp64 r, out its fp64 z; else both are float
void lsb_k_amg32_dense(unsigned nc, unsigned lanes, int ends64, const float *cinv, const void *b, void *out,
                       const struct lsb_pcg_state *st, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  const unsigned g = amg32_grid((unsigned long long)nc * lanes);
  if (ends64)
    LANES_DISPATCH(lanes, (k_amg32_dense<L, true, true><<<g, AMG32_WG, 0, s>>>(nc, cinv, b, out, st)));
  else
    LANES_DISPATCH(lanes, (k_amg32_dense<L, false, false><<<g, AMG32_WG, 0, s>>>(nc, cinv, b, out, st)));
}

} // extern "C"
