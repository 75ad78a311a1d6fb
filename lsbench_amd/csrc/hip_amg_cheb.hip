// The Chebyshev smoother of the AMG V-cycle (opts.amg_smoother = LSB_AMG_SMOOTH_CHEB) on interleaved blocks of
// KP = 2, 4 or 8 columns: hip_amg.hip's k_amg_cheb / k_amg_cheb_first in the layout and on the rounding rule of
// hip_mrhs_amg.hip (driver: amg_cycle in hip_amg_drv.c).  The rest of the cycle on blocks -- residual,
// restriction, prolongation, the dense coarse solve -- is hip_mrhs_amg.hip's, whatever the smoother.
//
// Rounding rule: per column exactly the single kernel's arithmetic -- a row's sums are block_row_product's
// (hip_mrhs_k.h), and lane 0 applies amg_cheb_dir (hip_amg_cheb.h), then y = x + d.  A column of the block has the
// BITS of the single-column cycle; columns never mix.  The direction block d is updated in place (row i reads
// only d_i) and is not read on a step with c1 == 0.
//
// Records: with REC the step leaves, per workgroup, one record of 2 KP doubles -- b_c . y_c per column, then
// b_c . b_c per column -- in the format k_mrhs_update_p reads (wg_sum_records<2 KP>: fixed order, no
// atomics).  On the fine level's last post-smoothing step b is the residual block and y is z, so AMG-PCG on
// blocks keeps having no dot-product launch.
//
// Gating: a no-op once st->running == 0 (NULL: always run); the state is never written.
#include "hip_kcommon.h"
#include "hip_mrhs_k.h"
#include "hip_amg_cheb.h"

// rows dealt to the workgroups in contiguous, XCD-contiguous ranges as k_amg_csr_m deals them
template <int L, int KP, bool REC>
__global__ __launch_bounds__(WG) void k_amg_cheb_m(unsigned n, unsigned rows_per_wg, const int *__restrict__ offs,
                                                   const int *__restrict__ cols, const double *__restrict__ vals,
                                                   const double *xin, const double *b, const double *dinv, double c1,
                                                   double c2, double *d, double *y, double *__restrict__ records,
                                                   const lsb_mrhs_state *st) {
  constexpr int H = KP / 2;
  constexpr unsigned SLOTS = WG / L;
  constexpr int ND = REC ? 2 * KP : 1;
  if (st && !st->running)
    return;
  const unsigned tid = threadIdx.x, slot = tid / L, l = tid % L;
  const unsigned w = xcd_contiguous_wg();
  const unsigned ra = min(w * rows_per_wg, n), rb = min(ra + rows_per_wg, n);
  const d2v *x2 = (const d2v *)xin, *b2 = (const d2v *)b;
  d2v *y2 = (d2v *)y, *d2 = (d2v *)d;
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
      const double m = dinv[r];
#pragma unroll
      for (int h = 0; h < H; h++) {
        const d2v bv = b2[o + h], xv = x2[o + h];
        d2v dv = {0.0, 0.0};
        if (c1 != 0.0)
          dv = d2[o + h];
        dv.x = amg_cheb_dir(c1, c2, m, bv.x, a[2 * h], dv.x);
        dv.y = amg_cheb_dir(c1, c2, m, bv.y, a[2 * h + 1], dv.y);
        d2[o + h] = dv;
        d2v s;
        s.x = xv.x + dv.x;
        s.y = xv.y + dv.y;
        if constexpr (REC) {
          dot[2 * h] = fma(bv.x, s.x, dot[2 * h]);
          dot[2 * h + 1] = fma(bv.y, s.y, dot[2 * h + 1]);
          dot[KP + 2 * h] = fma(bv.x, bv.x, dot[KP + 2 * h]);
          dot[KP + 2 * h + 1] = fma(bv.y, bv.y, dot[KP + 2 * h + 1]);
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

// step 0 from the zero guess, D = (c2 dinv) .* B and X = D: a stream at 16 B per lane
template <int KP>
__global__ __launch_bounds__(WG) void k_amg_cheb_first_m(unsigned n, const double *__restrict__ b,
                                                         const double *__restrict__ dinv, double c2,
                                                         double *__restrict__ d, double *__restrict__ x,
                                                         const lsb_mrhs_state *st) {
  constexpr int H = KP / 2;
  if (st && !st->running)
    return;
  const size_t npair = (size_t)n * H, gsz = (size_t)gridDim.x * WG;
  const d2v *b2 = (const d2v *)b;
  d2v *x2 = (d2v *)x, *d2 = (d2v *)d;
  for (size_t j = (size_t)blockIdx.x * WG + threadIdx.x; j < npair; j += gsz) {
    const d2v bv = b2[j];
    const double m = dinv[j / H];
    d2v v;
    v.x = amg_cheb_dir(0.0, c2, m, bv.x, 0.0, 0.0);
    v.y = amg_cheb_dir(0.0, c2, m, bv.y, 0.0, 0.0);
    d2[j] = v;
    x2[j] = v;
  }
}

// --------------------------------------------------------------------------
// Launchers (C ABI).  kp: 2, 4 or 8.
// --------------------------------------------------------------------------
template <int KP, bool REC>
static void amg_cheb_launch(const struct lsb_amg_mat *m, unsigned g, const double *xin, const double *b,
                            const double *dinv, double c1, double c2, double *d, double *y, double *records,
                            const struct lsb_mrhs_state *st, hipStream_t s) {
  ROW_KERNEL_LAUNCH(m->lanes, (k_amg_cheb_m<L, KP, REC>), g, s, m->rows, m->offs, m->cols, m->vals, xin, b, dinv, c1, c2,
                    d, y, records, st);
}

extern "C" {

void lsb_k_amg_cheb_first_m(unsigned kp, unsigned n, const double *b, const double *dinv, double c2, double *d,
                            double *x, const struct lsb_mrhs_state *st, void *stream) {
  if (n)
    KP_DISPATCH(kp, (k_amg_cheb_first_m<KP><<<sweep_grid(n, kp), WG, 0, (hipStream_t)stream>>>(n, b, dinv, c2, d, x,
                                                                                               st)));
}

void lsb_k_amg_cheb_m(unsigned kp, const struct lsb_amg_mat *m, const double *xin, const double *b,
                      const double *dinv, double c1, double c2, double *d, double *y, double *records,
                      unsigned *nrecords, const struct lsb_mrhs_state *st, void *stream) {
  if (!m->rows) {
    if (records)
      errx(EXIT_FAILURE, "lsb_k_amg_cheb_m: records of a matrix without rows");
    return;
  }
  hipStream_t s = (hipStream_t)stream;
  const unsigned g = lsb_k_spmm_grid(m->rows, row_lanes(m->lanes));
  if (nrecords)
    *nrecords = g;
  if (records)
    KP_DISPATCH(kp, (amg_cheb_launch<KP, true>(m, g, xin, b, dinv, c1, c2, d, y, records, st, s)));
  else
    KP_DISPATCH(kp, (amg_cheb_launch<KP, false>(m, g, xin, b, dinv, c1, c2, d, y, NULL, st, s)));
}

} // extern "C"
