// The fp32 V-cycle on blocks of right-hand sides: hip_amg_f32.hip's cycle on interleaved blocks of KP = 2, 4 or 8
// columns (driver: amg_cycle in hip_amg_drv.c, the fourth flavour; its caller: hip_rich_m_drv.c).  The schedule, the
// launch count, the lane counts and the ping-pong parity are the single-column cycle's.
//
// Layout: the matrices are hip_amg_f32.hip's packed 8-byte words {column, float bits}, minv and the coarse inverse its
// float arrays -- shared by all columns.  A level vector is a block of interleaved floats, element (i, c) at i KP + c,
// so a gather of row `col` is KP contiguous floats (8, 16 or 32 bytes, aligned to their size).  The two ends are fp64
// blocks in hip_mrhs.hip's layout: the caller's R and Z.
//
// One load of the entry word serves KP fmafs: a block of columns streams every matrix of the hierarchy once.
//
// Rounding rule: per column exactly hip_amg_f32.hip's --
//   1. lane l of a row's L lanes takes the entries l, l + L, ... in storage order: a_c = fmaf(val_j, x[col_j][c], a_c);
//   2. the L lane sums are folded by the xor butterfly L/2, ..., 1 with float additions;
//   3. lane 0 finishes in float -- SWEEP: fmaf(minv_i, b_ic - s_c, x_ic); RESID: b_ic - s_c; SPMV: s_c;
//      ADDP: y_ic + s_c.
// IN64 kernels (the fine level's first step; the coarse solve of a one-level hierarchy) round the fp64 block R once --
// the first step keeps the float copy, which every later step of the level reads -- and OUT64 kernels (the fine
// level's last sweep; that coarse solve) store their float results widened to fp64 straight into Z.  With the level's
// own lane count a column of the block therefore has the BITS of lsb_k_amg32_* on that column alone, whatever the
// other columns hold: columns never mix, so a NaN stays in its column.
//
// Gating: every kernel takes a const lsb_mrhs_state * and is a no-op once running == 0 (NULL: always run); none writes
// the state.  Frozen columns are computed along with the rest and nobody reads them.  No atomics, no allocation, no
// synchronisation.  Not built: the Chebyshev smoother, multicolour Gauss-Seidel, the one-launch tail.
#include "hip_kcommon.h"
#include "hip_mrhs_k.h"

#define AMG32M_HIDDEN __attribute__((visibility("hidden")))
#define AMG32_WG 256

typedef unsigned long long amg32_ent; // {col : 32 low, float bits : 32 high}
typedef float f2v __attribute__((ext_vector_type(2)));
typedef float f4v __attribute__((ext_vector_type(4)));

// row i of a float block <-> KP registers: one 8-byte access (KP = 2), or KP / 4 16-byte ones
template <int KP> __device__ __forceinline__ void frow_load(const float *v, size_t i, float (&o)[KP]) {
  if constexpr (KP == 2) {
    const f2v t = ((const f2v *)v)[i];
    o[0] = t.x, o[1] = t.y;
  } else {
#pragma unroll
    for (int h = 0; h < KP / 4; h++) {
      const f4v t = ((const f4v *)v)[i * (KP / 4) + h];
      o[4 * h] = t.x, o[4 * h + 1] = t.y, o[4 * h + 2] = t.z, o[4 * h + 3] = t.w;
    }
  }
}
template <int KP> __device__ __forceinline__ void frow_store(float *v, size_t i, const float (&o)[KP]) {
  if constexpr (KP == 2) {
    ((f2v *)v)[i] = f2v{o[0], o[1]};
  } else {
#pragma unroll
    for (int h = 0; h < KP / 4; h++)
      ((f4v *)v)[i * (KP / 4) + h] = f4v{o[4 * h], o[4 * h + 1], o[4 * h + 2], o[4 * h + 3]};
  }
}
// row i of an fp64 block, rounded to float once per element / a float row widened (exact)
template <int KP> __device__ __forceinline__ void drow_load_f32(const double *v, size_t i, float (&o)[KP]) {
  double t[KP];
  row_load<KP>(v, i, t);
#pragma unroll
  for (int k = 0; k < KP; k++)
    o[k] = (float)t[k];
}
template <int KP> __device__ __forceinline__ void drow_store_f32(double *v, size_t i, const float (&o)[KP]) {
  double t[KP];
#pragma unroll
  for (int k = 0; k < KP; k++)
    t[k] = (double)o[k];
  row_store<KP>(v, i, t);
}

// rule 2 on KP sums
template <int L, int KP> __device__ __forceinline__ void amg32m_fold(float (&a)[KP]) {
#pragma unroll
  for (int o = L / 2; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < KP; k++)
      a[k] += __shfl_xor(a[k], o, L);
  }
}

// y64 (OUT64) takes the result in the place of y
template <int L, int KP, int MODE, bool OUT64>
__global__ __launch_bounds__(AMG32_WG) void k_amg32_csr_m(unsigned n, const int *__restrict__ offs,
                                                          const amg32_ent *__restrict__ ent, const float *xin,
                                                          const float *b, const float *__restrict__ minv, float *y,
                                                          double *y64, const lsb_mrhs_state *st) {
  if (st && !st->running)
    return;
  const unsigned long long stride = (unsigned long long)gridDim.x * AMG32_WG; // a multiple of L: groups stay whole
  for (unsigned long long g = (unsigned long long)blockIdx.x * AMG32_WG + threadIdx.x; g / L < n; g += stride) {
    const unsigned i = (unsigned)(g / L), lane = (unsigned)(g % L);
    float a[KP];
#pragma unroll
    for (int k = 0; k < KP; k++)
      a[k] = 0.0f;
    const int e1 = offs[i + 1];
    for (int e = offs[i] + (int)lane; e < e1; e += L) {
      const amg32_ent w = ent[e];
      const float v = __uint_as_float((unsigned)(w >> 32));
      float xv[KP];
      frow_load<KP>(xin, (unsigned)w, xv);
#pragma unroll
      for (int k = 0; k < KP; k++)
        a[k] = fmaf(v, xv[k], a[k]);
    }
    amg32m_fold<L, KP>(a);
    if (lane == 0) {
      float o[KP];
      if constexpr (MODE == LSB_AMG_SWEEP) {
        float bv[KP], xv[KP];
        frow_load<KP>(b, i, bv);
        frow_load<KP>(xin, i, xv);
        const float m = minv[i];
#pragma unroll
        for (int k = 0; k < KP; k++)
          o[k] = fmaf(m, bv[k] - a[k], xv[k]);
      } else if constexpr (MODE == LSB_AMG_RESID) {
        float bv[KP];
        frow_load<KP>(b, i, bv);
#pragma unroll
        for (int k = 0; k < KP; k++)
          o[k] = bv[k] - a[k];
      } else if constexpr (MODE == LSB_AMG_SPMV) {
#pragma unroll
        for (int k = 0; k < KP; k++)
          o[k] = a[k];
      } else {
        float yv[KP];
        frow_load<KP>(y, i, yv);
#pragma unroll
        for (int k = 0; k < KP; k++)
          o[k] = yv[k] + a[k];
      }
      if constexpr (OUT64)
        drow_store_f32<KP>(y64, i, o);
      else
        frow_store<KP>(y, i, o);
    }
  }
}

// X = minv .* B from the zero guess; IN64: B is the fp64 block R, rounded once, the copy kept in b32
template <int KP, bool IN64>
__global__ __launch_bounds__(AMG32_WG) void k_amg32_first_m(unsigned n, const void *__restrict__ b,
                                                            const float *__restrict__ minv, float *__restrict__ x,
                                                            float *__restrict__ b32, const lsb_mrhs_state *st) {
  if (st && !st->running)
    return;
  for (unsigned i = blockIdx.x * AMG32_WG + threadIdx.x; i < n; i += gridDim.x * AMG32_WG) {
    float bv[KP], xv[KP];
    if constexpr (IN64) {
      drow_load_f32<KP>((const double *)b, i, bv);
      frow_store<KP>(b32, i, bv);
    } else
      frow_load<KP>((const float *)b, i, bv);
    const float m = minv[i];
#pragma unroll
    for (int k = 0; k < KP; k++)
      xv[k] = m * bv[k];
    frow_store<KP>(x, i, xv);
  }
}

// the coarse solve: a row of the dense nc x nc inverse times the block, rules 1 and 2; IN64 / OUT64: a hierarchy of
// one level, from R to Z
template <int L, int KP, bool IN64, bool OUT64>
__global__ __launch_bounds__(AMG32_WG) void k_amg32_dense_m(unsigned nc, const float *__restrict__ c,
                                                            const void *__restrict__ b, void *__restrict__ out,
                                                            const lsb_mrhs_state *st) {
  if (st && !st->running)
    return;
  for (unsigned g = blockIdx.x * AMG32_WG + threadIdx.x; g / L < nc; g += gridDim.x * AMG32_WG) {
    const unsigned i = g / L, lane = g % L;
    const float *ci = c + (size_t)i * nc;
    float a[KP];
#pragma unroll
    for (int k = 0; k < KP; k++)
      a[k] = 0.0f;
    for (unsigned j = lane; j < nc; j += L) {
      const float v = ci[j];
      float bv[KP];
      if constexpr (IN64)
        drow_load_f32<KP>((const double *)b, j, bv);
      else
        frow_load<KP>((const float *)b, j, bv);
#pragma unroll
      for (int k = 0; k < KP; k++)
        a[k] = fmaf(v, bv[k], a[k]);
    }
    amg32m_fold<L, KP>(a);
    if (lane == 0) {
      if constexpr (OUT64)
        drow_store_f32<KP>((double *)out, i, a);
      else
        frow_store<KP>((float *)out, i, a);
    }
  }
}

// --------------------------------------------------------------------------
// Launchers (hidden, declared in hip_solver.h).  kp: 2, 4 or 8; lanes: 2 .. 64, a power of two; grids as
// hip_amg_f32.hip's.
// --------------------------------------------------------------------------
static unsigned amg32m_grid(unsigned long long threads) {
  const unsigned long long g = (threads + AMG32_WG - 1) / AMG32_WG;
  return g > 16384ull ? 16384u : (g ? (unsigned)g : 1u);
}

template <int KP, int MODE, bool OUT64>
static void amg32m_csr_launch(const struct amg_mat32 *m, const float *xin, const float *b, const float *minv, float *y,
                              double *y64, const struct lsb_mrhs_state *st, hipStream_t s) {
  const unsigned g = amg32m_grid((unsigned long long)m->rows * m->lanes);
  LANES_DISPATCH(m->lanes, (k_amg32_csr_m<L, KP, MODE, OUT64><<<g, AMG32_WG, 0, s>>>(m->rows, m->offs, m->ent, xin, b,
                                                                                    minv, y, y64, st)));
}

extern "C" {

AMG32M_HIDDEN void lsb_k_amg32_first_m(unsigned kp, unsigned n, int in64, const void *b, const float *minv, float *x,
                                       float *b32, const struct lsb_mrhs_state *st, void *stream) {
  if (!n)
    return;
  hipStream_t s = (hipStream_t)stream;
  if (in64)
    KP_DISPATCH(kp, (k_amg32_first_m<KP, true><<<amg32m_grid(n), AMG32_WG, 0, s>>>(n, b, minv, x, b32, st)));
  else
    KP_DISPATCH(kp, (k_amg32_first_m<KP, false><<<amg32m_grid(n), AMG32_WG, 0, s>>>(n, b, minv, x, b32, st)));
}

AMG32M_HIDDEN void lsb_k_amg32_csr_m(unsigned kp, int mode, const struct amg_mat32 *m, const float *xin,
                                     const float *b, const float *minv, float *y, double *y64,
                                     const struct lsb_mrhs_state *st, void *stream) {
  if (!m->rows)
    return;
  hipStream_t s = (hipStream_t)stream;
  if (y64 && mode != LSB_AMG_SWEEP)
    errx(EXIT_FAILURE, "lsb_k_amg32_csr_m: only a sweep writes fp64");
  switch (mode) {
  case LSB_AMG_SWEEP:
    if (y64)
      KP_DISPATCH(kp, (amg32m_csr_launch<KP, LSB_AMG_SWEEP, true>(m, xin, b, minv, y, y64, st, s)));
    else
      KP_DISPATCH(kp, (amg32m_csr_launch<KP, LSB_AMG_SWEEP, false>(m, xin, b, minv, y, y64, st, s)));
    break;
  case LSB_AMG_RESID:
    KP_DISPATCH(kp, (amg32m_csr_launch<KP, LSB_AMG_RESID, false>(m, xin, b, minv, y, y64, st, s)));
    break;
  case LSB_AMG_SPMV:
    KP_DISPATCH(kp, (amg32m_csr_launch<KP, LSB_AMG_SPMV, false>(m, xin, b, minv, y, y64, st, s)));
    break;
  case LSB_AMG_ADDP:
    KP_DISPATCH(kp, (amg32m_csr_launch<KP, LSB_AMG_ADDP, false>(m, xin, b, minv, y, y64, st, s)));
    break;
  default:
    errx(EXIT_FAILURE, "lsb_k_amg32_csr_m: no mode %d", mode);
  }
}

// ends64: a hierarchy of one level -- b is the fp64 block R, out the fp64 block Z; else both are float blocks
AMG32M_HIDDEN void lsb_k_amg32_dense_m(unsigned kp, unsigned nc, unsigned lanes, int ends64, const float *cinv,
                                       const void *b, void *out, const struct lsb_mrhs_state *st, void *stream) {
  if (!nc)
    return;
  hipStream_t s = (hipStream_t)stream;
  const unsigned g = amg32m_grid((unsigned long long)nc * lanes);
  if (ends64)
    KP_DISPATCH(kp, LANES_DISPATCH(lanes, (k_amg32_dense_m<L, KP, true, true><<<g, AMG32_WG, 0, s>>>(nc, cinv, b, out,
                                                                                                    st))));
  else
    KP_DISPATCH(kp, LANES_DISPATCH(lanes, (k_amg32_dense_m<L, KP, false, false><<<g, AMG32_WG, 0, s>>>(nc, cinv, b,
                                                                                                      out, st))));
}

} // extern "C"
