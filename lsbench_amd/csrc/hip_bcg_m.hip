// Block-CG under a preconditioner that is an operator: the kernels lsb_hip_solver_solve_block_precond[_dev] adds to
// hip_bcg.hip's (driver: the second half of hip_bcg_drv.c).  The method is hip_bcg.hip's BCGrQ with D^-1 replaced by a
// symmetric M^-1 -- FSAI's G^T G, or the V-cycle -- so the preconditioned block is a stored operand Z:
//
//   start: Z = M^-1 B ; G = B^T Z, bb_c = b_c . b_c (k_bcgm_gram<START>) ; L L^T = G, sigma = L^T (k_bcg_small<START>)
//          W = B sigma^-1, P = Z sigma^-1, X = 0 (k_bcgm_start)
//   iter:  Q = S P, Gamma = P^T Q                                        k_bcg_spmm            (hip_bcg.hip)
//          xi = Gamma^-1, xs = xi sigma                                  k_bcg_small<GAMMA>    (hip_bcg.hip)
//          X += P xs, W~ = W - Q xi                                      k_bcgm_pass_a
//          Z~ = M^-1 W~, G = W~^T Z~, H = W~^T W~                        the V-cycle, then k_bcgm_gram ; or
//                                                                        T = G W~ (k_spmm_csr), then k_bcgm_gt_gram
//          rr, the stop test, L L^T = G, zeta = L^T, sigma = zeta sigma  k_bcg_small<G>        (hip_bcg.hip)
//          W = W~ zeta^-1, P = Z~ zeta^-1 + P zeta^T                     k_bcgm_pass_b
//
// Row by row w_r z_c is not symmetric, only its sum over the rows is: the kernels accumulate the upper triangle r <= c
// and k_bcg_small mirrors it, as it does for every record.  The records have the layouts of hip_bcg.hip's -- G's
// triangle then H's (k_bcg_pass_a's), or G's triangle then b_c . b_c (k_bcg_init's) -- so k_bcg_small reads them
// unchanged.  Layout, row ownership, uniform loads of the small matrices, one record per workgroup and no atomics, and
// the gate on st->running: all as in hip_bcg.hip.
#include "hip_kcommon.h"
#include "hip_mrhs_k.h"

#define BS LSB_MRHS_MAX // stride of the small matrices in the state

// X += P xs ; W~ = W - Q xi, in place.  No records: the Gram sums need Z~, which does not exist yet.
template <int KP>
__global__ __launch_bounds__(WG) void k_bcgm_pass_a(unsigned n, double *__restrict__ w, const double *__restrict__ q,
                                                    const double *__restrict__ p, double *__restrict__ x,
                                                    const lsb_blockcg_state *__restrict__ st) {
  if (!st->running)
    return;
  const size_t gsz = (size_t)gridDim.x * WG;
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += gsz) {
    double wv[KP], qv[KP], pv[KP], xv[KP];
    row_load<KP>(w, i, wv);
    row_load<KP>(q, i, qv);
    row_load<KP>(p, i, pv);
    row_load<KP>(x, i, xv);
#pragma unroll
    for (int c = 0; c < KP; c++) {
#pragma unroll
      for (int r = 0; r < KP; r++)
        xv[c] = fma(pv[r], st->xs[r * BS + c], xv[c]);
    }
    row_store<KP>(x, i, xv);
#pragma unroll
    for (int c = 0; c < KP; c++) {
#pragma unroll
      for (int r = 0; r < KP; r++)
        wv[c] = fma(-qv[r], st->xi[r * BS + c], wv[c]);
    }
    row_store<KP>(w, i, wv);
  }
}

// Two blocks A and Z of the same rows -> one record per workgroup.  In the loop: the upper triangles of A^T Z, then of
// A^T A (k_bcg_pass_a's layout), gated.  START: the upper triangle of A^T Z, then a_c . a_c per column (k_bcg_init's
// layout), not gated -- the state it would look at is written behind it.
template <int KP, bool START>
__global__ __launch_bounds__(WG) void k_bcgm_gram(unsigned n, const double *__restrict__ a,
                                                  const double *__restrict__ z, double *__restrict__ records,
                                                  const lsb_blockcg_state *__restrict__ st) {
  constexpr int T = tri_of(KP), W = START ? T + KP : 2 * T;
  __shared__ double sred[4 * W];
  if constexpr (!START) {
    if (!st->running)
      return;
  }
  const size_t gsz = (size_t)gridDim.x * WG;
  double acc[W];
#pragma unroll
  for (int k = 0; k < W; k++)
    acc[k] = 0.0;
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += gsz) {
    double av[KP], zv[KP];
    row_load<KP>(a, i, av);
    row_load<KP>(z, i, zv);
#pragma unroll
    for (int r = 0; r < KP; r++) {
#pragma unroll
      for (int c = r; c < KP; c++) {
        acc[tri_at(KP, r, c)] = fma(av[r], zv[c], acc[tri_at(KP, r, c)]);
        if constexpr (!START)
          acc[T + tri_at(KP, r, c)] = fma(av[r], av[c], acc[T + tri_at(KP, r, c)]);
      }
      if constexpr (START)
        acc[T + r] = fma(av[r], av[r], acc[T + r]);
    }
  }
  wg_sum_store<W>(acc, sred, records + (size_t)blockIdx.x * W);
}

// --------------------------------------------------------------------------
// FSAI's second product with the Gram sums riding in it: Z~ = G^T T by the row rule (block_row_product,
// hip_mrhs_k.h), so Z~ has the bits of lsb_hip_solver_spmm_dev's rule on the same T.  Every lane of the row's group
// then loads the row of W~ and takes its entries of the two upper triangles (the dealt triangle, hip_mrhs_k.h;
// k_bcg_spmm's scheme for P^T Q).  One record of 2 T doubles per workgroup (pass A's layout), rows dealt
// XCD-contiguously.  `offs`, `cols`, `vals`: the CSR of G^T.
// --------------------------------------------------------------------------
template <int L, int KP>
__global__ __launch_bounds__(WG) void k_bcgm_gt_gram(unsigned n, unsigned rows_per_wg, const int *__restrict__ offs,
                                                     const int *__restrict__ cols, const double *__restrict__ vals,
                                                     const double *__restrict__ t, const double *__restrict__ wt,
                                                     double *__restrict__ z, double *__restrict__ records,
                                                     const lsb_blockcg_state *__restrict__ st) {
  constexpr int T = tri_of(KP), NA = tri_dealt(KP, L);
  constexpr unsigned SLOTS = WG / L;
  __shared__ double sred[4 * 2 * T];
  const unsigned tid = threadIdx.x, slot = tid / L, l = tid % L;
  const unsigned w = xcd_contiguous_wg();
  const unsigned ra = min(w * rows_per_wg, n), rb = min(ra + rows_per_wg, n);
  const int stopped = !st->running;
  double g[2][NA]; // W~^T Z~ and W~^T W~, this lane's entries
#pragma unroll
  for (int k = 0; k < NA; k++)
    g[0][k] = 0.0, g[1][k] = 0.0;
  for (unsigned base = ra; base < rb; base += SLOTS) {
    const unsigned r = base + slot;
    double a[KP];
    block_row_product<L, KP>(offs, cols, vals, t, r, r < rb, l, a);
    if (stopped)
      return;
    if (r < rb) {
      double wr[KP];
      row_load<KP>(wt, r, wr);
      if (l == 0)
        row_store<KP>(z, r, a);
      tri_dealt_fma<L, KP>(wr, {a, wr}, l, g);
    }
  }
  if (stopped)
    return;
  tri_dealt_store<L, KP>(g, sred, records + (size_t)w * 2 * T);
}

// W = B zinv (zinv = sigma^-1, upper triangular), P = Z zinv, X = 0.  Not gated: X = 0 is the answer of a block that
// does not run (maxit = 0).
template <int KP>
__global__ __launch_bounds__(WG) void k_bcgm_start(unsigned n, const double *__restrict__ b,
                                                   const double *__restrict__ z, double *__restrict__ w,
                                                   double *__restrict__ p, double *__restrict__ x,
                                                   const lsb_blockcg_state *__restrict__ st) {
  const size_t gsz = (size_t)gridDim.x * WG;
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += gsz) {
    double bv[KP], zv[KP], wv[KP], pv[KP], zero[KP];
    row_load<KP>(b, i, bv);
    row_load<KP>(z, i, zv);
#pragma unroll
    for (int c = 0; c < KP; c++) {
      double s = 0.0, u = 0.0;
#pragma unroll
      for (int r = 0; r <= c; r++) {
        s = fma(bv[r], st->zinv[r * BS + c], s);
        u = fma(zv[r], st->zinv[r * BS + c], u);
      }
      wv[c] = s, pv[c] = u, zero[c] = 0.0;
    }
    row_store<KP>(w, i, wv);
    row_store<KP>(p, i, pv);
    row_store<KP>(x, i, zero);
  }
}

// W = W~ zinv (upper triangular) ; P = Z~ zinv + P zeta^T (zeta upper triangular)
template <int KP>
__global__ __launch_bounds__(WG) void k_bcgm_pass_b(unsigned n, double *__restrict__ w, const double *__restrict__ z,
                                                    double *__restrict__ p,
                                                    const lsb_blockcg_state *__restrict__ st) {
  if (!st->running)
    return;
  const size_t gsz = (size_t)gridDim.x * WG;
  for (size_t i = (size_t)blockIdx.x * WG + threadIdx.x; i < n; i += gsz) {
    double wt[KP], zt[KP], pv[KP], wv[KP], pn[KP];
    row_load<KP>(w, i, wt);
    row_load<KP>(z, i, zt);
    row_load<KP>(p, i, pv);
#pragma unroll
    for (int c = 0; c < KP; c++) {
      double s = 0.0, u = 0.0;
#pragma unroll
      for (int r = 0; r <= c; r++) {
        s = fma(wt[r], st->zinv[r * BS + c], s);
        u = fma(zt[r], st->zinv[r * BS + c], u);
      }
      wv[c] = s;
#pragma unroll
      for (int r = c; r < KP; r++) // (P zeta^T)_c = sum_r p_r zeta[c][r], zeta[c][r] = 0 for r < c
        u = fma(pv[r], st->zeta[c * BS + r], u);
      pn[c] = u;
    }
    row_store<KP>(w, i, wv);
    row_store<KP>(p, i, pn);
  }
}

// --------------------------------------------------------------------------
// Launchers (C ABI).  kp: 2, 4 or 8; lanes: 2 .. 32, any other count takes a whole wavefront.
// --------------------------------------------------------------------------
template <int KP>
static void gt_gram_launch(unsigned lanes, unsigned g, unsigned n, const int *offs, const int *cols, const double *vals,
                           const double *t, const double *wt, double *z, double *records,
                           const struct lsb_blockcg_state *st, hipStream_t s) {
  ROW_KERNEL_LAUNCH(lanes, (k_bcgm_gt_gram<L, KP>), g, s, n, offs, cols, vals, t, wt, z, records, st);
}

extern "C" {

void lsb_k_blockcg_m_pass_a(unsigned kp, unsigned n, double *w, const double *q, const double *p, double *x,
                            const struct lsb_blockcg_state *st, void *stream) {
  KP_DISPATCH(kp, (k_bcgm_pass_a<KP><<<pass_grid(n), WG, 0, (hipStream_t)stream>>>(n, w, q, p, x, st)));
}

void lsb_k_blockcg_m_gram(unsigned kp, int start, unsigned n, const double *a, const double *z, double *records,
                          unsigned *nrecords, const struct lsb_blockcg_state *st, void *stream) {
  const unsigned g = pass_grid(n);
  *nrecords = g;
  if (start)
    KP_DISPATCH(kp, (k_bcgm_gram<KP, true><<<g, WG, 0, (hipStream_t)stream>>>(n, a, z, records, st)));
  else
    KP_DISPATCH(kp, (k_bcgm_gram<KP, false><<<g, WG, 0, (hipStream_t)stream>>>(n, a, z, records, st)));
}

void lsb_k_blockcg_m_gt_gram(unsigned kp, unsigned n, const int *offs, const int *cols, const double *vals,
                             unsigned lanes, const double *t, const double *wt, double *z, double *records,
                             unsigned *nrecords, const struct lsb_blockcg_state *st, void *stream) {
  const unsigned L = row_lanes(lanes), g = lsb_k_spmm_grid(n, L);
  *nrecords = g;
  KP_DISPATCH(kp, (gt_gram_launch<KP>(L, g, n, offs, cols, vals, t, wt, z, records, st, (hipStream_t)stream)));
}

void lsb_k_blockcg_m_start(unsigned kp, unsigned n, const double *b, const double *z, double *w, double *p, double *x,
                           const struct lsb_blockcg_state *st, void *stream) {
  KP_DISPATCH(kp, (k_bcgm_start<KP><<<pass_grid(n), WG, 0, (hipStream_t)stream>>>(n, b, z, w, p, x, st)));
}

void lsb_k_blockcg_m_pass_b(unsigned kp, unsigned n, double *w, const double *z, double *p,
                            const struct lsb_blockcg_state *st, void *stream) {
  KP_DISPATCH(kp, (k_bcgm_pass_b<KP><<<pass_grid(n), WG, 0, (hipStream_t)stream>>>(n, w, z, p, st)));
}

} // extern "C"
