// Multicolour Gauss-Seidel smoothing in the AMG V-cycle (opts.amg_smoother = LSB_AMG_SMOOTH_MCGS, --amg-smoother
// mcgs), in fp64 and in fp32.  The rows of a level are coloured on the host so that no stored off-diagonal entry
// couples two rows of one colour (lsb_amg_colour), and the level's matrix is copied with its rows regrouped colour
// by colour (lsb_csr_mcgs): the launch of colour c streams the contiguous rows [cbeg[c], cbeg[c + 1]) of that copy
// and rowid gives the row of the level a lane group reads and writes.  Column ids are the level's, so the vectors
// keep their numbering.
//
// A colour step c on (x, b), IN PLACE, touches only the rows i of colour c:
//     s_i = sum_j a_ij x_j     the row rule of hip_amg.hip's amg_row<L> / hip_amg_f32.hip's amg32_row<L>, restated
//                              here: lane l of the row's L takes the entries l, l + L, ... of the copied row in
//                              storage order through the fma chain, then the xor butterfly over the L lanes
//     x_i <- fma(dinv_i, b_i - s_i, x_i)      dinv_i = 1 / a_ii: the finish of a sweep with dinv in the place of minv
// A forward sweep is the colours 0 .. C - 1, each a launch; a backward sweep C - 1 .. 0.  Pre-smoothing is nu forward
// sweeps from the zero guess, post-smoothing nu backward sweeps (amg_cycle in hip_amg_drv.c): each is the adjoint of
// the other, so the cycle stays a symmetric positive definite preconditioner.
//
// Why in place is race-free: a row of colour c reads x_j of other colours, which this launch does not write, and its
// own x_i, which only its own lane group writes -- lane 0, after the butterfly has consumed every lane's loads (a
// group lies inside one wavefront).  x is read and written through the same pointer and so takes no __restrict__.
// lsb_mcgs_check asserts the colouring, the permutation and the copy on the host at every upload.  No atomics:
// z is bitwise repeatable.
//
// k_amg_mcgs_first / k_amg32_mcgs_first<IN64>: the very first launch of the pre-smoothing, element-wise over ALL rows:
// x_i = fma(dinv_i, b_i, 0) on colour 0 and x_i = 0 elsewhere -- the bits of the general step on a zeroed x, and it
// streams no matrix.  IN64 (the fine level of the fp32 cycle) reads the caller's fp64 r, rounds it once and keeps
// the float copy in b32, which every later launch of the level reads, as k_amg32_first does.
// k_amg32_mcgs<L, OUT64>: OUT64 launches (the fine level's last backward sweep) store the float result to the
// iterate -- later colours of the same sweep read it -- AND widened to the caller's fp64 z: no conversion launch.
// Every kernel is a no-op once the solve's state has left RUNNING.  Not built: blocks of columns, the one-launch tail.
#include "hip_kcommon.h"

#define MCGS_WG 256

typedef unsigned long long mcgs_ent; // fp32: {col : 32 low, float bits : 32 high} (lsb_csr_pack_f32)

// position p of the copy times x in fp64 (amg_row<L> of hip_amg.hip)
template <int L>
__device__ __forceinline__ double mcgs_row(const int *offs, const int *cols, const double *vals, const double *x,
                                           unsigned p, unsigned lane) {
  double acc = 0.0;
  const int e1 = offs[p + 1];
  for (int e = offs[p] + (int)lane; e < e1; e += L)
    acc = fma(vals[e], x[cols[e]], acc);
#pragma unroll
  for (int o = L / 2; o > 0; o >>= 1)
    acc += __shfl_xor(acc, o, L);
  return acc;
}

// the same in fp32 on packed entries (amg32_row<L> of hip_amg_f32.hip)
template <int L>
__device__ __forceinline__ float mcgs32_row(const int *offs, const mcgs_ent *ent, const float *x, unsigned p,
                                            unsigned lane) {
  float acc = 0.0f;
  const int e1 = offs[p + 1];
  for (int e = offs[p] + (int)lane; e < e1; e += L) {
    const mcgs_ent w = ent[e];
    acc = fmaf(__uint_as_float((unsigned)(w >> 32)), x[(unsigned)w], acc);
  }
#pragma unroll
  for (int o = L / 2; o > 0; o >>= 1)
    acc += __shfl_xor(acc, o, L);
  return acc;
}

// one colour: positions p0 .. p0 + cnt - 1 of the copy
template <int L>
__global__ __launch_bounds__(MCGS_WG) void k_amg_mcgs(unsigned p0, unsigned cnt, const int *__restrict__ rowid,
                                                      const int *__restrict__ offs, const int *__restrict__ cols,
                                                      const double *__restrict__ vals, double *x,
                                                      const double *__restrict__ b, const double *__restrict__ dinv,
                                                      const struct lsb_pcg_state *st) {
  if (st && st->status)
    return;
  const unsigned long long stride = (unsigned long long)gridDim.x * MCGS_WG; // a multiple of L: groups stay whole
  for (unsigned long long g = (unsigned long long)blockIdx.x * MCGS_WG + threadIdx.x; g / L < cnt; g += stride) {
    const unsigned p = p0 + (unsigned)(g / L), lane = (unsigned)(g % L);
    const double s = mcgs_row<L>(offs, cols, vals, x, p, lane);
    if (lane == 0) {
      const unsigned i = (unsigned)rowid[p];
      x[i] = fma(dinv[i], b[i] - s, x[i]);
    }
  }
}

__global__ __launch_bounds__(MCGS_WG) void k_amg_mcgs_first(unsigned n, const unsigned char *__restrict__ colour,
                                                            const double *__restrict__ b,
                                                            const double *__restrict__ dinv, double *__restrict__ x,
                                                            const struct lsb_pcg_state *st) {
  if (st && st->status)
    return;
  for (unsigned i = blockIdx.x * MCGS_WG + threadIdx.x; i < n; i += gridDim.x * MCGS_WG)
    x[i] = colour[i] == 0 ? fma(dinv[i], b[i], 0.0) : 0.0;
}

template <int L, bool OUT64>
__global__ __launch_bounds__(MCGS_WG) void k_amg32_mcgs(unsigned p0, unsigned cnt, const int *__restrict__ rowid,
                                                        const int *__restrict__ offs,
                                                        const mcgs_ent *__restrict__ ent, float *x,
                                                        const float *__restrict__ b, const float *__restrict__ dinv,
                                                        double *__restrict__ z64, const struct lsb_pcg_state *st) {
  if (st && st->status)
    return;
  const unsigned long long stride = (unsigned long long)gridDim.x * MCGS_WG; // a multiple of L: groups stay whole
  for (unsigned long long g = (unsigned long long)blockIdx.x * MCGS_WG + threadIdx.x; g / L < cnt; g += stride) {
    const unsigned p = p0 + (unsigned)(g / L), lane = (unsigned)(g % L);
    const float s = mcgs32_row<L>(offs, ent, x, p, lane);
    if (lane == 0) {
      const unsigned i = (unsigned)rowid[p];
      const float v = fmaf(dinv[i], b[i] - s, x[i]);
      x[i] = v;
      if (OUT64)
        z64[i] = (double)v;
    }
  }
}

template <bool IN64>
__global__ __launch_bounds__(MCGS_WG) void k_amg32_mcgs_first(unsigned n, const unsigned char *__restrict__ colour,
                                                              const void *__restrict__ b,
                                                              const float *__restrict__ dinv, float *__restrict__ x,
                                                              float *__restrict__ b32,
                                                              const struct lsb_pcg_state *st) {
  if (st && st->status)
    return;
  for (unsigned i = blockIdx.x * MCGS_WG + threadIdx.x; i < n; i += gridDim.x * MCGS_WG) {
    const float bi = IN64 ? (float)((const double *)b)[i] : ((const float *)b)[i];
    if (IN64)
      b32[i] = bi;
    x[i] = colour[i] == 0 ? fmaf(dinv[i], bi, 0.0f) : 0.0f;
  }
}

// --------------------------------------------------------------------------
// Launchers (C ABI; declared in lsb_impl.h).  m: the colour-sorted copy, lanes 2 .. 64 by the level's own count;
// [p0, p1): the colour's range of positions, inside [0, m->rows).
// --------------------------------------------------------------------------
static unsigned mcgs_grid(unsigned long long threads) {
  const unsigned long long g = (threads + MCGS_WG - 1) / MCGS_WG;
  return g > 16384ull ? 16384u : (g ? (unsigned)g : 1u);
}

extern "C" {

void lsb_k_amg_mcgs_first(unsigned n, const unsigned char *colour, const double *b, const double *dinv, double *x,
                          const struct lsb_pcg_state *st, void *stream) {
  if (n)
    k_amg_mcgs_first<<<mcgs_grid(n), MCGS_WG, 0, (hipStream_t)stream>>>(n, colour, b, dinv, x, st);
}

void lsb_k_amg_mcgs(const struct lsb_amg_mat *m, const int *rowid, unsigned p0, unsigned p1, double *x,
                    const double *b, const double *dinv, const struct lsb_pcg_state *st, void *stream) {
  if (p0 > p1 || p1 > m->rows)
    errx(EXIT_FAILURE, "lsb_k_amg_mcgs: positions %u .. %u of %u rows", p0, p1, m->rows);
  if (p0 == p1)
    return;
  hipStream_t s = (hipStream_t)stream;
  const unsigned cnt = p1 - p0, g = mcgs_grid((unsigned long long)cnt * m->lanes);
  LANES_DISPATCH(m->lanes, (k_amg_mcgs<L><<<g, MCGS_WG, 0, s>>>(p0, cnt, rowid, m->offs, m->cols, m->vals, x, b, dinv,
                                                               st)));
}

void lsb_k_amg32_mcgs_first(unsigned n, int in64, const unsigned char *colour, const void *b, const float *dinv,
                            float *x, float *b32, const struct lsb_pcg_state *st, void *stream) {
  if (!n)
    return;
  hipStream_t s = (hipStream_t)stream;
  if (in64)
    k_amg32_mcgs_first<true><<<mcgs_grid(n), MCGS_WG, 0, s>>>(n, colour, b, dinv, x, b32, st);
  else
    k_amg32_mcgs_first<false><<<mcgs_grid(n), MCGS_WG, 0, s>>>(n, colour, b, dinv, x, b32, st);
}

// z64 != NULL: the result goes to x and, widened, to z64
void lsb_k_amg32_mcgs(const struct amg_mat32 *m, const int *rowid, unsigned p0, unsigned p1, float *x, const float *b,
                      const float *dinv, double *z64, const struct lsb_pcg_state *st, void *stream) {
  if (p0 > p1 || p1 > m->rows)
    errx(EXIT_FAILURE, "lsb_k_amg32_mcgs: positions %u .. %u of %u rows", p0, p1, m->rows);
  if (p0 == p1)
    return;
  hipStream_t s = (hipStream_t)stream;
  const unsigned cnt = p1 - p0, g = mcgs_grid((unsigned long long)cnt * m->lanes);
  if (z64)
    LANES_DISPATCH(m->lanes, (k_amg32_mcgs<L, true><<<g, MCGS_WG, 0, s>>>(p0, cnt, rowid, m->offs, m->ent, x, b, dinv,
                                                                         z64, st)));
  else
    LANES_DISPATCH(m->lanes, (k_amg32_mcgs<L, false><<<g, MCGS_WG, 0, s>>>(p0, cnt, rowid, m->offs, m->ent, x, b, dinv,
                                                                          z64, st)));
}

} // extern "C"
