// Successive right-hand sides: the sweeps of the projection onto earlier solutions (DESIGN.md section 4,
// "Successive right-hand sides"; host side: hip_seq_drv.c).  The basis is m <= LSB_SEQ_MAX_DEPTH pairs (x~_k, S x~_k),
// vector-major with an even leading dimension ld as GMRES's V is, so every column starts on a 16-byte boundary.
//
// All four are HBM-bound passes over m + 1 (dots, combine), 2 m + 2 (orth) or 4 (store) vectors.  They are templated
// on m: the loops over the basis are unrolled and the accumulators are registers at m = 16; none may use scratch
// (tests/test_seq_resources.py).  A lane takes two neighbouring rows per turn.  The pair is written as two 8-byte
// accesses, which is all the alignment a caller's vector promises; the compiler merges them into one 16-byte access,
// and gfx950's global memory takes that at any 8-byte address -- one kernel per m, whatever the operands' alignment.
// A turn's loads of ALL its streams are issued before anything waits for one: left alone, the scheduler sinks each
// load to its use to save registers (k_seq_orth<8> then runs with one to three loads outstanding), so a scheduling
// barrier stands between a turn's loads and its arithmetic, and the kernels spend the registers: k_seq_orth<16> holds
// 34 16-byte loads per lane in flight.  Nothing is atomic: a lane adds its rows in index order, the workgroup sums by
// wg_sum and writes one record, lsb_k_reduce_final adds the records in an order fixed by their number.  k_seq_orth's
// sums are k_seq_dots's on the vectors it has just written, expression for expression, so the two agree bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lsb_impl.h"
#include "hip_wg.h"

#define SEQ_MAX LSB_SEQ_MAX_DEPTH
typedef double sq_d2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ sq_d2 sq_ld(const double *__restrict__ p, size_t i) {
  sq_d2 r;
  r.x = p[2 * i], r.y = p[2 * i + 1];
  return r;
}
__device__ __forceinline__ void sq_st(double *__restrict__ p, size_t i, sq_d2 v) { p[2 * i] = v.x, p[2 * i + 1] = v.y; }
// nothing is scheduled across: the loads in front of it are all issued before the arithmetic behind it begins
__device__ __forceinline__ void sq_loads_issued() { __builtin_amdgcn_sched_barrier(0); }
// the one expression every sum of this file grows by
__device__ __forceinline__ double sq_acc(sq_d2 a, sq_d2 b, double acc) { return fma(a.y, b.y, fma(a.x, b.x, acc)); }

// one record of M partials per workgroup: sum_i X[k][i] v[i]
template <int M>
__global__ __launch_bounds__(WG) void k_seq_dots(unsigned n, const double *__restrict__ X, size_t ld,
                                                 const double *__restrict__ v, double *__restrict__ partials) {
  __shared__ double sred[4 * M];
  double acc[M];
#pragma unroll
  for (int k = 0; k < M; k++)
    acc[k] = 0.0;
  const size_t npair = n / 2;
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < npair; i += (size_t)gridDim.x * WG) {
    const sq_d2 vi = sq_ld(v, i);
    sq_d2 xv[M];
#pragma unroll
    for (int k = 0; k < M; k++)
      xv[k] = sq_ld(X + (size_t)k * ld, i);
    sq_loads_issued();
#pragma unroll
    for (int k = 0; k < M; k++)
      acc[k] = sq_acc(xv[k], vi, acc[k]);
  }
  if ((n & 1u) && blockIdx.x == 0 && threadIdx.x == 0) { // the odd last row
    const double vi = v[n - 1];
#pragma unroll
    for (int k = 0; k < M; k++)
      acc[k] = fma(X[(size_t)k * ld + (n - 1)], vi, acc[k]);
  }
  wg_sum<M>(acc, sred);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < M; k++)
      partials[(size_t)blockIdx.x * M + k] = acc[k];
  }
}

// x0_i = sum_k alpha_k X[k][i]: an fma chain in ascending k from 0.0
template <int M>
__global__ __launch_bounds__(WG) void k_seq_combine(unsigned n, const double *__restrict__ X, size_t ld,
                                                    const double *__restrict__ alpha, double *__restrict__ x0) {
  double a[M];
#pragma unroll
  for (int k = 0; k < M; k++)
    a[k] = alpha[k];
  const size_t npair = n / 2;
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < npair; i += (size_t)gridDim.x * WG) {
    sq_d2 xv[M];
#pragma unroll
    for (int k = 0; k < M; k++)
      xv[k] = sq_ld(X + (size_t)k * ld, i);
    sq_loads_issued();
    sq_d2 s = {0.0, 0.0};
#pragma unroll
    for (int k = 0; k < M; k++)
      s.x = fma(a[k], xv[k].x, s.x), s.y = fma(a[k], xv[k].y, s.y);
    sq_st(x0, i, s);
  }
  if ((n & 1u) && blockIdx.x == 0 && threadIdx.x == 0) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < M; k++)
      s = fma(a[k], X[(size_t)k * ld + (n - 1)], s);
    x0[n - 1] = s;
  }
}

// One Gram-Schmidt pass on the pair (d, w = S d), in place: d -= sum_k beta_k X[k], w -= sum_k beta_k SX[k] in
// ascending k; and of what the row has just produced, one record of M + 2 partials per workgroup: X[k] . w' (the
// next pass's coefficients), d' . w', and -- from before the update -- d . w.
template <int M>
__global__ __launch_bounds__(WG) void k_seq_orth(unsigned n, const double *__restrict__ X,
                                                 const double *__restrict__ SX, size_t ld,
                                                 const double *__restrict__ beta, double *__restrict__ d,
                                                 double *__restrict__ w, double *__restrict__ partials) {
  __shared__ double sred[4 * (M + 2)];
  double b[M], acc[M + 2];
#pragma unroll
  for (int k = 0; k < M; k++)
    b[k] = -beta[k];
#pragma unroll
  for (int k = 0; k < M + 2; k++)
    acc[k] = 0.0;
  const size_t npair = n / 2;
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < npair; i += (size_t)gridDim.x * WG) {
    sq_d2 vd = sq_ld(d, i), vw = sq_ld(w, i);
    sq_d2 xv[M], sv[M];
#pragma unroll
    for (int k = 0; k < M; k++)
      xv[k] = sq_ld(X + (size_t)k * ld, i);
#pragma unroll
    for (int k = 0; k < M; k++)
      sv[k] = sq_ld(SX + (size_t)k * ld, i);
    sq_loads_issued();
    acc[M + 1] = sq_acc(vd, vw, acc[M + 1]);
#pragma unroll
    for (int k = 0; k < M; k++) {
      vd.x = fma(b[k], xv[k].x, vd.x), vd.y = fma(b[k], xv[k].y, vd.y);
      vw.x = fma(b[k], sv[k].x, vw.x), vw.y = fma(b[k], sv[k].y, vw.y);
    }
    sq_st(d, i, vd), sq_st(w, i, vw);
#pragma unroll
    for (int k = 0; k < M; k++)
      acc[k] = sq_acc(xv[k], vw, acc[k]);
    acc[M] = sq_acc(vd, vw, acc[M]);
  }
  if ((n & 1u) && blockIdx.x == 0 && threadIdx.x == 0) {
    const size_t j = n - 1;
    double di = d[j], wi = w[j];
    acc[M + 1] = fma(di, wi, acc[M + 1]);
#pragma unroll
    for (int k = 0; k < M; k++)
      di = fma(b[k], X[(size_t)k * ld + j], di), wi = fma(b[k], SX[(size_t)k * ld + j], wi);
    d[j] = di, w[j] = wi;
#pragma unroll
    for (int k = 0; k < M; k++)
      acc[k] = fma(X[(size_t)k * ld + j], wi, acc[k]);
    acc[M] = fma(di, wi, acc[M]);
  }
  wg_sum<M + 2>(acc, sred);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < M + 2; k++)
      partials[(size_t)blockIdx.x * (M + 2) + k] = acc[k];
  }
}

// The new pair: xs = d / sqrt(nu), sxs = w / sqrt(nu) with nu = d . w read from the device, and the record
// (nu0, nu, stored).  nu not finite or not > 0: the record alone.
__global__ __launch_bounds__(WG) void k_seq_store(unsigned n, const double *__restrict__ d,
                                                  const double *__restrict__ w, double *__restrict__ xs,
                                                  double *__restrict__ sxs, const double *__restrict__ nu,
                                                  const double *__restrict__ nu0, double *__restrict__ rec) {
  const double v = *nu;
  const bool ok = v > 0.0 && v < __builtin_huge_val(); // (a NaN compares false)
  if (blockIdx.x == 0 && threadIdx.x == 0)
    rec[0] = *nu0, rec[1] = v, rec[2] = ok ? 1.0 : 0.0;
  if (!ok)
    return;
  const double s = sqrt(v);
  const size_t npair = n / 2;
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < npair; i += (size_t)gridDim.x * WG) {
    const sq_d2 vd = sq_ld(d, i), vw = sq_ld(w, i);
    sq_d2 a, c;
    a.x = vd.x / s, a.y = vd.y / s;
    c.x = vw.x / s, c.y = vw.y / s;
    sq_st(xs, i, a), sq_st(sxs, i, c);
  }
  if ((n & 1u) && blockIdx.x == 0 && threadIdx.x == 0)
    xs[n - 1] = d[n - 1] / s, sxs[n - 1] = w[n - 1] / s;
}

// one pair of rows per lane until the cap on the workgroups of a streaming launch, grid-stride beyond it
static unsigned seq_grid(unsigned n) {
  unsigned g = (n / 2 + WG - 1) / WG;
  if (g > LSB_STREAM_GRID_CAP)
    g = LSB_STREAM_GRID_CAP;
  return g ? g : 1;
}

static void seq_check_m(unsigned m, const char *who) {
  if (m == 0 || m > SEQ_MAX)
    errx(EXIT_FAILURE, "hip_cdna4: %s: %u basis vectors (1 .. %d)", who, m, SEQ_MAX);
}

// the launch of K<m> for m = 1 .. 16
#define SEQ_CASE(K, M, ...)                                                                                            \
  case M:                                                                                                              \
    K<M><<<g, WG, 0, (hipStream_t)stream>>>(__VA_ARGS__);                                                              \
    break;
#define SEQ_DISPATCH(K, ...)                                                                                           \
  switch (m) {                                                                                                         \
    SEQ_CASE(K, 1, __VA_ARGS__) SEQ_CASE(K, 2, __VA_ARGS__) SEQ_CASE(K, 3, __VA_ARGS__) SEQ_CASE(K, 4, __VA_ARGS__)    \
    SEQ_CASE(K, 5, __VA_ARGS__) SEQ_CASE(K, 6, __VA_ARGS__) SEQ_CASE(K, 7, __VA_ARGS__) SEQ_CASE(K, 8, __VA_ARGS__)    \
    SEQ_CASE(K, 9, __VA_ARGS__) SEQ_CASE(K, 10, __VA_ARGS__) SEQ_CASE(K, 11, __VA_ARGS__)                              \
    SEQ_CASE(K, 12, __VA_ARGS__) SEQ_CASE(K, 13, __VA_ARGS__) SEQ_CASE(K, 14, __VA_ARGS__)                             \
    SEQ_CASE(K, 15, __VA_ARGS__) SEQ_CASE(K, 16, __VA_ARGS__)                                                          \
  }

extern "C" {

unsigned lsb_k_seq_grid(unsigned n) { return seq_grid(n); }

void lsb_k_seq_dots(unsigned n, unsigned m, const double *X, size_t ld, const double *v, double *partials,
                    double *alpha, void *stream) {
  seq_check_m(m, "lsb_k_seq_dots");
  const unsigned g = seq_grid(n);
  SEQ_DISPATCH(k_seq_dots, n, X, ld, v, partials)
  lsb_k_reduce_final(partials, g, m, alpha, 0, NULL, stream);
}

void lsb_k_seq_combine(unsigned n, unsigned m, const double *X, size_t ld, const double *alpha, double *x0,
                       void *stream) {
  seq_check_m(m, "lsb_k_seq_combine");
  const unsigned g = seq_grid(n);
  SEQ_DISPATCH(k_seq_combine, n, X, ld, alpha, x0)
}

void lsb_k_seq_orth(unsigned n, unsigned m, const double *X, const double *SX, size_t ld, const double *beta,
                    double *d, double *w, double *partials, double *out, void *stream) {
  seq_check_m(m, "lsb_k_seq_orth");
  const unsigned g = seq_grid(n);
  SEQ_DISPATCH(k_seq_orth, n, X, SX, ld, beta, d, w, partials)
  lsb_k_reduce_final(partials, g, m + 2, out, 0, NULL, stream);
}

void lsb_k_seq_store(unsigned n, const double *d, const double *w, double *xs, double *sxs, const double *nu,
                     const double *nu0, double *rec, void *stream) {
  k_seq_store<<<seq_grid(n), WG, 0, (hipStream_t)stream>>>(n, d, w, xs, sxs, nu, nu0, rec);
}

} // extern "C"
