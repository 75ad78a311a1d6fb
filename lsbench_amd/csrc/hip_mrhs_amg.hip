// Several right-hand sides under AMG: the V-cycle of hip_amg.hip on interleaved blocks of KP = 2, 4 or 8
// columns (driver: amg_cycle in hip_amg_drv.c).  The PCG sweeps around it are hip_mrhs.hip's with z as a block of
// its own: an iteration is SpMM, k_mrhs_update_xr<KP, true>, the cycle, k_mrhs_update_p<KP, true>.
//
// Layout: hip_mrhs.hip's -- element (i, c) at i KP + c, 16-byte aligned -- on every level of the hierarchy.
// Every matrix of the hierarchy (A, P, R of a level, the dense coarse inverse) is streamed once for all KP
// columns; a gather of row `col` is KP contiguous doubles.
//
// Rounding rule: each column's arithmetic is hip_amg.hip's amg_row<L> / amg_finish<MODE> exactly -- a row's sums are
// block_row_product's (hip_mrhs_k.h), which per column is amg_row<L>'s chain and butterfly, and lane 0 applies the
// same finishing expression.  With the level's own `lanes` a column of the block therefore has the BITS of the
// single-column cycle, whatever the other columns hold; columns never mix, so a NaN stays in its column.
//
// Records: the SWEEP form with REC leaves, per workgroup, one record of 2 KP doubles -- b_c . y_c per column,
// then b_c . b_c per column -- in the format k_mrhs_update_p reads (wg_sum_records<2 KP>: fixed order, no
// atomics).  On the fine level's last sweep b is the residual block and y is z, so (r.z, r.r) of every column
// come out of the launch that writes z and the iteration has no dot-product launch.  A one-level hierarchy
// has no sweep: hip_mrhs.hip's k_amg_dot2_m forms the records behind the dense solve.
//
// Gating: every kernel of the cycle takes a const lsb_mrhs_state * and is a no-op once running == 0 (NULL:
// always run); none writes the state, so the word is never set and tested in the same launch.  Frozen columns
// are computed along with the rest and nobody reads them.
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
    block_row_product<L, KP>(offs, cols, vals, xin, r, r < rb, l, a);
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

// --------------------------------------------------------------------------
// Launchers (C ABI).  kp: 2, 4 or 8.
// --------------------------------------------------------------------------
template <int KP, int MODE, bool REC>
static void amg_csr_launch(const struct lsb_amg_mat *m, unsigned g, const double *xin, const double *b,
                           const double *minv, double *y, double *records, const struct lsb_mrhs_state *st,
                           hipStream_t s) {
  ROW_KERNEL_LAUNCH(m->lanes, (k_amg_csr_m<L, KP, MODE, REC>), g, s, m->rows, m->offs, m->cols, m->vals, xin, b, minv, y,
                    records, st);
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
  const unsigned g = lsb_k_spmm_grid(m->rows, row_lanes(m->lanes));
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
  const unsigned Lr = row_lanes(lanes), g = div_up(nc, WG / Lr);
  KP_DISPATCH(kp, LANES_DISPATCH(lanes, (k_amg_dense_m<L, KP><<<g, WG, 0, s>>>(nc, cinv, b, out, st))));
}

} // extern "C"
