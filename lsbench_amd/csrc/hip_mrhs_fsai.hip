// FSAI-preconditioned PCG on blocks of right-hand sides (opts.fsai_blocks; driver: hip_mrhs_drv.c): the two row
// kernels that stand between the SpMM and k_mrhs_update_p<KP, true>.  z = G^T (G r) is a block of its own, and the
// x / r sweep rides in the two products as in the single-column form (hip_fsai.hip), at width KP.  An iteration is
// FOUR launches:
//   1  k_spmm_csr (hip_mrhs.hip, as it is):  Q = S P and the records of p_c . q_c
//   2  k_mrhs_fsai_xr_gr:   alpha_c = rz_c / pq_c, k_mrhs_update_xr's breakdown decision and bookkeeping;
//                           x_c += alpha_c p_c on the own rows;  T = G R' with r'_c = fma(-alpha_c, q_c, r_c) formed
//                           IN THE GATHER of G's rows.  r is only read.
//   3  k_mrhs_fsai_gt_dots: Z = G^T T;  r'_c stored IN PLACE for the own rows, by the same fma -- the bits launch 2
//                           used;  one record per workgroup of (r'_c . z_c, then r'_c . r'_c)
//   4  k_mrhs_update_p<KP, true> (hip_mrhs.hip, as it is):  the stop test on those records, p = z + beta p
// Launch 2 gathers r of other workgroups' rows, so nothing overwrites r there; launch 3 gathers t only and touches r
// on its own rows alone.  There is one residual block, no parity of buffers: a column frozen in any iteration leaves
// its r where init, a warm start and a verify restart look for it.
//
// Blocks are hip_mrhs.hip's: interleaved, element (i, c) at i KP + c.  L lanes per row and one rounding rule, the
// SpMM's: block_row_product (hip_mrhs_k.h).  Launch 3 calls it; launch 2 keeps the same loop and butterfly written
// out, because what it gathers is not a stored block but r' = fma(-alpha, q, r).
//
// Gating as in hip_mrhs.hip: launch 2 decides per column from the status words and the records (every workgroup
// the same decision, workgroup 0 writes) and may CLEAR `running`, which it never reads; launch 3 is a no-op once
// `running` is 0 and never writes it.  A column whose status is not RUNNING is frozen: none of its x, r, t, z is
// stored.  alpha_c travels from launch 2 to launch 3 in the column's state (alpha[parity], written by workgroup 0),
// and a column is active in launch 3 exactly when launch 2 left it RUNNING.
#include "hip_kcommon.h"
#include "hip_mrhs_k.h"

// a value every lane of the wavefront holds, moved into scalar registers
__device__ __forceinline__ double wave_uniform(double v) {
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)),
                          __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

template <int L, int KP>
__global__ __launch_bounds__(WG) void k_mrhs_fsai_xr_gr(unsigned n, unsigned rows_per_wg,
                                                        const int *__restrict__ goffs, const int *__restrict__ gcols,
                                                        const double *__restrict__ gvals, const double *__restrict__ p,
                                                        const double *__restrict__ q, double *__restrict__ x,
                                                        const double *__restrict__ r, double *__restrict__ t,
                                                        lsb_mrhs_state *__restrict__ st, int parity,
                                                        const double *__restrict__ pq_parts, unsigned npq) {
  constexpr int H = KP / 2;
  constexpr unsigned SLOTS = WG / L;
  __shared__ double sred[4 * KP], spq[KP], salpha[KP];
  __shared__ int sact[KP], sent[KP];
  const unsigned tid = threadIdx.x, slot = tid / L, l = tid % L;
  const unsigned w = xcd_contiguous_wg();
  const unsigned ra = min(w * rows_per_wg, n), rb = min(ra + rows_per_wg, n);
  wg_sum_records<KP>(pq_parts, npq, sred, spq);
  if (tid < KP) { // k_mrhs_update_xr's decision and bookkeeping
    lsb_pcg_state *c = &st->c[tid];
    const int entered = c->status == LSB_STATUS_RUNNING;
    int act = 0;
    double alpha = 0.0;
    if (entered) {
      const double pq = spq[tid];
      if (!(pq != 0.0) || !isfinite(pq)) { // the same decision in every workgroup
        if (blockIdx.x == 0)
          c->status = LSB_STATUS_BREAKDOWN;
      } else {
        alpha = c->rz[parity] / pq;
        act = 1;
        if (blockIdx.x == 0)
          c->pq = pq, c->alpha[parity] = alpha; // alpha: what launch 3 forms r' with
      }
    }
    sent[tid] = entered, sact[tid] = act, salpha[tid] = alpha;
  }
  __syncthreads();
  int any = 0, anyent = 0;
#pragma unroll
  for (int k = 0; k < KP; k++)
    any |= sact[k], anyent |= sent[k];
  if (blockIdx.x == 0 && tid == 0 && anyent) {
    st->nspmm += 1; // the SpMM in front of this launch worked
    if (!any)
      st->running = 0; // the last columns broke down: launch 3 is a no-op
  }
  if (!any)
    return;
  double al[KP]; // 0 for a frozen column: its r' is its r
#pragma unroll
  for (int k = 0; k < KP; k++)
    al[k] = wave_uniform(salpha[k]);
  const d2v *p2 = (const d2v *)p, *q2 = (const d2v *)q, *r2 = (const d2v *)r;
  const d2v *x2 = (const d2v *)x;
  for (unsigned base = ra; base < rb; base += SLOTS) {
    const unsigned row = base + slot;
    double a[KP];
#pragma unroll
    for (int k = 0; k < KP; k++)
      a[k] = 0.0;
    if (row < rb) { // block_row_product's loop and butterfly (hip_mrhs_k.h) with r' formed in the gather
      const int j0 = goffs[row], j1 = goffs[row + 1];
      for (int j = j0 + (int)l; j < j1; j += L) {
        const double v = gvals[j];
        const size_t c = (size_t)gcols[j] * H;
        d2v qv[H], rv[H];
#pragma unroll
        for (int h = 0; h < H; h++)
          qv[h] = q2[c + h], rv[h] = r2[c + h];
#pragma unroll
        for (int h = 0; h < H; h++) {
          a[2 * h] = fma(v, fma(-al[2 * h], qv[h].x, rv[h].x), a[2 * h]);
          a[2 * h + 1] = fma(v, fma(-al[2 * h + 1], qv[h].y, rv[h].y), a[2 * h + 1]);
        }
      }
    }
#pragma unroll
    for (int off = L >> 1; off > 0; off >>= 1) {
#pragma unroll
      for (int k = 0; k < KP; k++)
        a[k] += __shfl_xor(a[k], off, 64);
    }
    if (row < rb && l == 0) {
      const size_t o = (size_t)row * H;
#pragma unroll
      for (int h = 0; h < H; h++) {
        const int a0 = sact[2 * h], a1 = sact[2 * h + 1];
        if (a0 | a1) {
          const d2v pv = p2[o + h];
          d2v xv = x2[o + h];
          xv.x = fma(al[2 * h], pv.x, xv.x), xv.y = fma(al[2 * h + 1], pv.y, xv.y);
          store_pairs({x, t}, {xv, d2v{a[2 * h], a[2 * h + 1]}}, o + h, a0, a1);
        }
      }
    }
  }
}

template <int L, int KP>
__global__ __launch_bounds__(WG) void k_mrhs_fsai_gt_dots(unsigned n, unsigned rows_per_wg,
                                                          const int *__restrict__ offs, const int *__restrict__ cols,
                                                          const double *__restrict__ vals, const double *__restrict__ t,
                                                          const double *__restrict__ q, double *r,
                                                          double *__restrict__ z, double *__restrict__ records,
                                                          const lsb_mrhs_state *__restrict__ st, int parity) {
  constexpr int H = KP / 2;
  constexpr unsigned SLOTS = WG / L;
  __shared__ double sred[8 * KP];
  const unsigned tid = threadIdx.x, slot = tid / L, l = tid % L;
  const unsigned w = xcd_contiguous_wg();
  const unsigned ra = min(w * rows_per_wg, n), rb = min(ra + rows_per_wg, n);
  // the words travel with the first row's loads; nothing is stored before `running` is tested, and no launch that
  // runs beside this one writes it
  const int stopped = !st->running;
  int act[KP];
  double al[KP];
#pragma unroll
  for (int k = 0; k < KP; k++) {
    act[k] = st->c[k].status == LSB_STATUS_RUNNING;
    al[k] = act[k] ? st->c[k].alpha[parity] : 0.0;
  }
  const d2v *q2 = (const d2v *)q;
  double dot[2 * KP]; // r'.z per column, then r'.r'
#pragma unroll
  for (int k = 0; k < 2 * KP; k++)
    dot[k] = 0.0;
  for (unsigned base = ra; base < rb; base += SLOTS) {
    const unsigned row = base + slot;
    double a[KP];
    block_row_product<L, KP>(offs, cols, vals, t, row, row < rb, l, a);
    if (stopped)
      return;
    if (row < rb && l == 0) {
      const size_t o = (size_t)row * H;
#pragma unroll
      for (int h = 0; h < H; h++) {
        const d2v qv = q2[o + h], rv = ((const d2v *)r)[o + h];
        d2v rn;
        rn.x = fma(-al[2 * h], qv.x, rv.x), rn.y = fma(-al[2 * h + 1], qv.y, rv.y);
        const d2v zv = {a[2 * h], a[2 * h + 1]};
        if (act[2 * h] | act[2 * h + 1])
          store_pairs({r, z}, {rn, zv}, o + h, act[2 * h], act[2 * h + 1]);
        dot[2 * h] = fma(rn.x, zv.x, dot[2 * h]);
        dot[2 * h + 1] = fma(rn.y, zv.y, dot[2 * h + 1]);
        dot[KP + 2 * h] = fma(rn.x, rn.x, dot[KP + 2 * h]);
        dot[KP + 2 * h + 1] = fma(rn.y, rn.y, dot[KP + 2 * h + 1]);
      }
    }
  }
  if (stopped)
    return;
  wg_sum<2 * KP>(dot, sred);
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 2 * KP; k++)
      records[(size_t)w * 2 * KP + k] = dot[k];
  }
}

// --------------------------------------------------------------------------
// Launchers (C ABI).  kp: 2, 4 or 8; lanes: 2 .. 32, any other count takes a whole wavefront.
// --------------------------------------------------------------------------
template <int KP>
static void xr_gr_launch(unsigned lanes, unsigned g, unsigned n, const int *goffs, const int *gcols,
                         const double *gvals, const double *p, const double *q, double *x, const double *r, double *t,
                         struct lsb_mrhs_state *st, int parity, const double *pq_parts, unsigned npq, hipStream_t s) {
  ROW_KERNEL_LAUNCH(lanes, (k_mrhs_fsai_xr_gr<L, KP>), g, s, n, goffs, gcols, gvals, p, q, x, r, t, st, parity, pq_parts,
                    npq);
}

template <int KP>
static void gt_dots_launch(unsigned lanes, unsigned g, unsigned n, const int *offs, const int *cols, const double *vals,
                           const double *t, const double *q, double *r, double *z, double *records,
                           const struct lsb_mrhs_state *st, int parity, hipStream_t s) {
  ROW_KERNEL_LAUNCH(lanes, (k_mrhs_fsai_gt_dots<L, KP>), g, s, n, offs, cols, vals, t, q, r, z, records, st, parity);
}

extern "C" {

void lsb_k_mrhs_fsai_xr_gr(unsigned kp, unsigned n, const int *goffs, const int *gcols, const double *gvals,
                           unsigned lanes, const double *p, const double *q, double *x, const double *r, double *t,
                           struct lsb_mrhs_state *st, int parity, const double *pq_parts, unsigned npq, void *stream) {
  const unsigned L = row_lanes(lanes), g = lsb_k_spmm_grid(n, L);
  KP_DISPATCH(kp, (xr_gr_launch<KP>(L, g, n, goffs, gcols, gvals, p, q, x, r, t, st, parity, pq_parts, npq,
                                    (hipStream_t)stream)));
}

void lsb_k_mrhs_fsai_gt_dots(unsigned kp, unsigned n, const int *offs, const int *cols, const double *vals,
                             unsigned lanes, const double *t, const double *q, double *r, double *z, double *records,
                             unsigned *nrecords, const struct lsb_mrhs_state *st, int parity, void *stream) {
  const unsigned L = row_lanes(lanes), g = lsb_k_spmm_grid(n, L);
  *nrecords = g;
  KP_DISPATCH(kp, (gt_dots_launch<KP>(L, g, n, offs, cols, vals, t, q, r, z, records, st, parity,
                                      (hipStream_t)stream)));
}

} // extern "C"
