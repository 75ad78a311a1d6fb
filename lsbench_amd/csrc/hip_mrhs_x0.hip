// A batch of right-hand sides from an initial guess X0 (lsb_hip_solver_solve_multi_x0_dev; driver: mrhs_batch in
// hip_mrhs_drv.c): the two sweeps around the SpMM r = b - S x0.  The state behind them is k_mrhs_init_state's
// (hip_mrhs.hip), handed the records of b.b.  Layout, records and reductions: hip_mrhs.hip, hip_mrhs_k.h.
#include "hip_kcommon.h"
#include "hip_mrhs_k.h"

// --------------------------------------------------------------------------
// x holds X0, the SpMM with bres = b leaves r = b - S x0, and the state is built from scratch -- the restart
// kernels of a verify round consume a state that exists.  A column whose x0 = 0 must come out with the bits of a
// batch from zero: r = b then, and p, b.b, r.z and r.r are formed by k_mrhs_init's expressions, over the same
// grid, into records of the same width.
// --------------------------------------------------------------------------
// before the SpMM: one record (0 per column, then b.b per column) per workgroup
template <int KP>
__global__ __launch_bounds__(WG) void k_mrhs_x0_bb(unsigned n, const double *__restrict__ b,
                                                   double *__restrict__ bb_parts) {
  __shared__ double sred[8 * KP], sout[2 * KP];
  const size_t npair = (size_t)n * (KP / 2), gsz = (size_t)gridDim.x * WG;
  const d2v *b2 = (const d2v *)b;
  double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
  for (size_t j = (size_t)blockIdx.x * WG + threadIdx.x; j < npair; j += gsz) {
    const d2v bv = b2[j];
    acc[1][0] += bv.x * bv.x, acc[1][1] += bv.y * bv.y;
  }
  wg_sum_cols<KP, 2>(acc, sred, sout);
  if (threadIdx.x < 2 * KP)
    bb_parts[(size_t)blockIdx.x * 2 * KP + threadIdx.x] = sout[threadIdx.x];
}

// behind the SpMM: x_c = 0 for the columns with b_c = 0 (the rule of a batch from zero, whatever x0 holds); !Z:
// p = dinv .* r and one record (r.z per column, then r.r per column) per workgroup.  Z: the zeroing alone -- the
// cycle on r and k_amg_dot2_m<KP, true> follow.  r and p of every column are written: no state gates them yet.
template <int KP, bool Z>
__global__ __launch_bounds__(WG) void k_mrhs_x0_start(unsigned n, const double *__restrict__ r,
                                                      const double *__restrict__ dinv, double dc,
                                                      double *__restrict__ x, double *__restrict__ p,
                                                      const double *__restrict__ bb_parts, unsigned nbb,
                                                      double *__restrict__ partials2) {
  constexpr int H = KP / 2;
  __shared__ double sred[8 * KP], sbb[2 * KP], sout[2 * KP];
  const size_t gtid = (size_t)blockIdx.x * WG + threadIdx.x, gsz = (size_t)gridDim.x * WG;
  const size_t npair = (size_t)n * H;
  const d2v *r2 = (const d2v *)r;
  d2v *p2 = (d2v *)p;
  wg_sum_records<2 * KP>(bb_parts, nbb, sred, sbb);
  const unsigned c0 = (2u * threadIdx.x) % KP;
  const int z0 = sbb[KP + c0] == 0.0, z1 = sbb[KP + c0 + 1] == 0.0;
  double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
  if (!Z || (z0 | z1)) {
    for (size_t j = gtid; j < npair; j += gsz) {
      if constexpr (!Z) {
        const d2v rv = r2[j];
        const double d = dinv ? dinv[j / H] : dc;
        d2v pv;
        pv.x = d * rv.x, pv.y = d * rv.y;
        p2[j] = pv;
        acc[0][0] += rv.x * pv.x, acc[0][1] += rv.y * pv.y;
        acc[1][0] += rv.x * rv.x, acc[1][1] += rv.y * rv.y;
      }
      if (z0 | z1)
        store_pairs({x}, {d2v{0.0, 0.0}}, j, z0, z1);
    }
  }
  if constexpr (!Z) {
    wg_sum_cols<KP, 2>(acc, sred, sout);
    if (threadIdx.x < 2 * KP)
      partials2[(size_t)blockIdx.x * 2 * KP + threadIdx.x] = sout[threadIdx.x];
  }
}

// --------------------------------------------------------------------------
// Launchers (C ABI).  kp: 2, 4 or 8.
// --------------------------------------------------------------------------
extern "C" {

void lsb_k_mrhs_x0_bb(unsigned kp, unsigned n, const double *b, double *bb_parts, unsigned *nbb, void *stream) {
  const unsigned g = sweep_grid(n, kp);
  *nbb = g;
  KP_DISPATCH(kp, (k_mrhs_x0_bb<KP><<<g, WG, 0, (hipStream_t)stream>>>(n, b, bb_parts)));
}

void lsb_k_mrhs_x0_start(unsigned kp, unsigned n, const double *r, const double *dinv, double dc, double *x,
                         double *p, const double *bb_parts, unsigned nbb, double *partials2, unsigned *npartials,
                         void *stream) {
  const unsigned g = sweep_grid(n, kp);
  *npartials = g;
  KP_DISPATCH(kp, (k_mrhs_x0_start<KP, false><<<g, WG, 0, (hipStream_t)stream>>>(n, r, dinv, dc, x, p, bb_parts, nbb,
                                                                                 partials2)));
}

void lsb_k_amg_mrhs_x0_start(unsigned kp, unsigned n, double *x, const double *bb_parts, unsigned nbb, void *stream) {
  KP_DISPATCH(kp, (k_mrhs_x0_start<KP, true><<<sweep_grid(n, kp), WG, 0, (hipStream_t)stream>>>(
                      n, NULL, NULL, 0.0, x, NULL, bb_parts, nbb, NULL)));
}

} // extern "C"
