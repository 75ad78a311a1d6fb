// What the kernel files of several right-hand sides (hip_mrhs.hip, hip_mrhs_x0.hip, hip_mrhs_fsai.hip, hip_mrhs_amg.hip,
// hip_amg_cheb.hip, hip_amg_f32_m.hip, hip_rich_m.hip, hip_bcg.hip, hip_bcg_m.hip, hip_direct_m.hip, hip_direct_tm.hip) share: the 16-byte pair of the interleaved blocks and its store gated
// per column, the fixed-order reductions of their per-column records, the verify round's decision, the row rule of
// their CSR row kernels (block_row_product), the Gram triangle dealt over a row's lanes, and the launchers' dispatch
// on the batch width and on the lanes per row.  Included by those files only, after hip_kcommon.h.
#ifndef LSB_HIP_MRHS_K_H
#define LSB_HIP_MRHS_K_H
#include "hip_kcommon.h"

typedef double d2v __attribute__((ext_vector_type(2)));

// Sum `nparts` records of width W (one per workgroup of an earlier launch) per component into sout[W]: thread
// t takes component t mod W of records t / W, t / W + WG / W, ...; butterfly over the lanes of a wave that
// share the component, the four waves through LDS in fixed order.  sred: 4 W doubles.
template <int W>
__device__ __forceinline__ void wg_sum_records(const double *__restrict__ parts, unsigned nparts, double *sred,
                                               double *sout) {
  static_assert(W >= 2 && W <= 32 && (W & (W - 1)) == 0, "record width");
  const unsigned t = threadIdx.x, k = t % W;
  double v = 0.0;
  for (unsigned i = t / W; i < nparts; i += WG / W)
    v += parts[(size_t)i * W + k];
#pragma unroll
  for (int off = 32; off >= W; off >>= 1)
    v += __shfl_xor(v, off, 64);
  __syncthreads(); // sred / sout may still be read from a previous call
  if ((t & 63) < W)
    sred[(t >> 6) * W + k] = v;
  __syncthreads();
  if (t < W)
    sout[t] = (sred[t] + sred[W + t]) + (sred[2 * W + t] + sred[3 * W + t]);
  __syncthreads();
}

// Per-column sums of NV quantities over the workgroup: lane t holds, for each quantity, the sums of its two
// columns (2 t mod KP, + 1).  sout[q KP + c]; sred: 4 NV KP doubles.
template <int KP, int NV>
__device__ __forceinline__ void wg_sum_cols(double (&v)[NV][2], double *sred, double *sout) {
  constexpr int H = KP / 2;
#pragma unroll
  for (int q = 0; q < NV; q++) {
#pragma unroll
    for (int off = 32; off >= H; off >>= 1) {
      v[q][0] += __shfl_xor(v[q][0], off, 64);
      v[q][1] += __shfl_xor(v[q][1], off, 64);
    }
  }
  const unsigned t = threadIdx.x, lane = t & 63, wave = t >> 6;
  constexpr int W = NV * KP;
  __syncthreads();
  if (lane < H) {
#pragma unroll
    for (int q = 0; q < NV; q++) {
      sred[wave * W + q * KP + 2 * lane] = v[q][0];
      sred[wave * W + q * KP + 2 * lane + 1] = v[q][1];
    }
  }
  __syncthreads();
  if (t < W)
    sout[t] = (sred[t] + sred[W + t]) + (sred[2 * W + t] + sred[3 * W + t]);
  __syncthreads();
}

// opts.verify: the recomputed residual of a column and whether a column called converged misses the tolerance
__device__ __forceinline__ double mrhs_true_relres(const lsb_pcg_state *c, double rr) {
  return c->bb > 0.0 ? sqrt(rr / c->bb) : -1.0;
}
__device__ __forceinline__ bool mrhs_misses(const lsb_pcg_state *c, double rr, double tol) {
  return c->status == LSB_STATUS_CONVERGED && c->bb > 0.0 && !(mrhs_true_relres(c, rr) <= tol);
}

// the restart decision of a verify round, per column into sact[KP]: the column was called converged, its
// recomputed residual (the sum of the records rr_parts) misses the tolerance, and a round and iterations are left.
// The same decision in every workgroup and in every launch of the round.  sred: 4 KP doubles, srr: KP.
template <int KP>
__device__ __forceinline__ void restart_decision(const lsb_mrhs_state *st, const double *rr_parts, unsigned nrr,
                                                 int more, double *sred, double *srr, int *sact) {
  wg_sum_records<KP>(rr_parts, nrr, sred, srr);
  if (threadIdx.x < KP) {
    const lsb_pcg_state *c = &st->c[threadIdx.x];
    sact[threadIdx.x] = more && c->iters < c->maxit && mrhs_misses(c, srr[threadIdx.x], st->tol);
  }
  __syncthreads();
}

// Store pair j of NB blocks where at least one of the pair's two columns is active (a0 | a1): both -> one 16-byte
// store per block, one -> its 8-byte half.  The half of a frozen column is never stored.
template <int NB>
__device__ __forceinline__ void store_pairs(double *const (&v)[NB], const d2v (&val)[NB], size_t j, int a0, int a1) {
  if (a0 & a1) {
#pragma unroll
    for (int b = 0; b < NB; b++)
      ((d2v *)v[b])[j] = val[b];
  } else if (a0) {
#pragma unroll
    for (int b = 0; b < NB; b++)
      v[b][2 * j] = val[b].x;
  } else {
#pragma unroll
    for (int b = 0; b < NB; b++)
      v[b][2 * j + 1] = val[b].y;
  }
}

// --------------------------------------------------------------------------
// THE ROW RULE of every CSR row kernel on blocks ("One rounding rule"): a[c] = (row `row` of the
// matrix) . (column c of the block x), L lanes per row.  Lane l reads (col, val) of its entries j0 + l, j0 + l + L,
// ... once each, in storage order, gathers the KP / 2 16-byte pairs of row `col` of x and runs the chain
// a[c] = fma(val_j, x_jc, a[c]), written with explicit fma(); the L lane sums are folded by the xor butterfly
// L/2, ..., 1, after which EVERY lane of the row's group holds the row's sums.  A lane whose row is out of range
// (in_range == false) reads nothing, contributes zeros and takes part in the butterfly.  Whoever calls this has the
// bits of k_spmm_csr -- of lsb_hip_solver_spmm_dev -- on the same operands.
// --------------------------------------------------------------------------
template <int L, int KP>
__device__ __forceinline__ void block_row_product(const int *offs, const int *cols, const double *vals, const double *x,
                                                  unsigned row, bool in_range, unsigned l, double (&a)[KP]) {
  constexpr int H = KP / 2;
  const d2v *x2 = (const d2v *)x;
#pragma unroll
  for (int k = 0; k < KP; k++)
    a[k] = 0.0;
  if (in_range) {
    const int j0 = offs[row], j1 = offs[row + 1];
    for (int j = j0 + (int)l; j < j1; j += L) {
      const double v = vals[j];
      const size_t c = (size_t)cols[j] * H;
#pragma unroll
      for (int h = 0; h < H; h++) {
        const d2v t = x2[c + h];
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
}

// --------------------------------------------------------------------------
// What the two block-CG kernel files (hip_bcg.hip, hip_bcg_m.hip) share: a lane of their streaming launches owns whole
// rows, and the Gram matrices leave a launch as records of their upper triangle.
// --------------------------------------------------------------------------
#define BCG_PASS_GRID 512 // workgroups of a streaming pass at the most (its consumer has ONE workgroup to sum them)

static_assert(BCG_PASS_GRID <= LSB_STREAM_GRID_CAP, "the driver sizes the passes' records by LSB_STREAM_GRID_CAP");

// (i, j), i <= j, in the upper triangle stored row by row
__host__ __device__ constexpr int tri_at(int KP, int i, int j) { return i * KP - i * (i - 1) / 2 + (j - i); }
__host__ __device__ constexpr int tri_of(int KP) { return KP * (KP + 1) / 2; }

// a row's KP doubles <-> KP / 2 16-byte accesses
template <int KP> __device__ __forceinline__ void row_load(const double *__restrict__ v, size_t i, double (&o)[KP]) {
  const d2v *v2 = (const d2v *)v + i * (KP / 2);
#pragma unroll
  for (int h = 0; h < KP / 2; h++) {
    const d2v t = v2[h];
    o[2 * h] = t.x, o[2 * h + 1] = t.y;
  }
}
template <int KP> __device__ __forceinline__ void row_store(double *__restrict__ v, size_t i, const double (&o)[KP]) {
  d2v *v2 = (d2v *)v + i * (KP / 2);
#pragma unroll
  for (int h = 0; h < KP / 2; h++)
    v2[h] = d2v{o[2 * h], o[2 * h + 1]};
}

// the workgroup's sums of W per-lane values -> dst[W]: wavefront butterfly, the four waves through LDS in fixed order
template <int W> __device__ __forceinline__ void wg_sum_store(double (&v)[W], double *sred /* 4 W */, double *dst) {
#pragma unroll
  for (int k = 0; k < W; k++) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
      v[k] += __shfl_xor(v[k], off, 64);
  }
  const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < W; k++)
      sred[wave * W + k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < W)
    dst[threadIdx.x] = (sred[threadIdx.x] + sred[W + threadIdx.x]) + (sred[2 * W + threadIdx.x] + sred[3 * W + threadIdx.x]);
}

// The DEALT TRIANGLE of the row kernels that carry Gram sums (k_bcg_spmm, k_bcgm_gt_gram).  After the row rule's
// butterfly every lane of a row's group holds the row, so the T = tri_of(KP) entries of the upper triangle of u^T v are
// dealt over the group's L lanes: lane l takes the entries t = l, l + L, ... and keeps ceil(T / L) running sums, not T.
__host__ __device__ constexpr int tri_dealt(int KP, int L) { return (tri_of(KP) + L - 1) / L; }

// one row's u_i v_j into this lane's entries of NT triangles, v = v[0], v[1], ... (KP doubles each)
template <int L, int KP, int NT, int NA>
__device__ __forceinline__ void tri_dealt_fma(const double (&u)[KP], const double *const (&v)[NT], unsigned l,
                                              double (&g)[NT][NA]) {
  static_assert(NA == tri_dealt(KP, L), "a lane's share of the triangle");
#pragma unroll
  for (int i = 0; i < KP; i++) {
#pragma unroll
    for (int j = i; j < KP; j++) {
      const int t = tri_at(KP, i, j); // a constant after unrolling
#pragma unroll
      for (int q = 0; q < NT; q++) { // (a select, no branch: every lane forms the sum, the entry's owner keeps it)
        const double s = fma(u[i], v[q][j], g[q][t / L]);
        g[q][t / L] = (unsigned)(t % L) == l ? s : g[q][t / L];
      }
    }
  }
}

// the workgroup's sums of NT dealt triangles -> one record of NT T doubles at dst, triangle after triangle: lanes of a
// wave with the same l hold the same entries (butterfly 32, ..., L), the four waves through LDS in fixed order.
// sred: 4 NT T doubles, not in use when the workgroup gets here.
template <int L, int KP, int NT, int NA>
__device__ __forceinline__ void tri_dealt_store(double (&g)[NT][NA], double *sred, double *dst) {
  constexpr int T = tri_of(KP), W = NT * T;
#pragma unroll
  for (int k = 0; k < NA; k++) {
#pragma unroll
    for (int off = 32; off >= L; off >>= 1) {
#pragma unroll
      for (int q = 0; q < NT; q++)
        g[q][k] += __shfl_xor(g[q][k], off, 64);
    }
  }
  const unsigned tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (lane < L) {
#pragma unroll
    for (int k = 0; k < NA; k++)
      if (k * L + (int)lane < T) {
#pragma unroll
        for (int q = 0; q < NT; q++)
          sred[wave * W + q * T + k * L + lane] = g[q][k];
      }
  }
  __syncthreads();
  if (tid < W)
    dst[tid] = (sred[tid] + sred[W + tid]) + (sred[2 * W + tid] + sred[3 * W + tid]);
}

// --------------------------------------------------------------------------
// What the two kernel files of the direct solver on blocks (hip_direct_m.hip, hip_direct_tm.hip) share: all running
// columns of a block have run the same number of rounds, so which round it is comes from any of them.
// --------------------------------------------------------------------------
// rounds the running columns have completed (0: round 1 is next)
template <int KP> __device__ __forceinline__ int dirm_round(const lsb_mrhs_state *__restrict__ st) {
  int it = 0;
#pragma unroll
  for (int c = KP - 1; c >= 0; c--)
    it = st->c[c].status == LSB_STATUS_RUNNING ? st->c[c].iters : it;
  return it;
}

// --------------------------------------------------------------------------
// host helpers of the launchers.  kp: 2, 4 or 8.
// --------------------------------------------------------------------------
// rows of a block-CG streaming pass: one row per lane and trip
static inline unsigned pass_grid(unsigned n) {
  unsigned g = div_up(n ? n : 1, WG);
  if (g > 256) {
    g = div_up(n, WG * 4);
    if (g < 256)
      g = 256;
  }
  return g > BCG_PASS_GRID ? BCG_PASS_GRID : g;
}

static unsigned kshift_of(unsigned kp) {
  if (kp != 2 && kp != 4 && kp != 8)
    errx(EXIT_FAILURE, "hip_mrhs: a batch is 2, 4 or 8 columns wide, not %u", kp);
  return kp == 2 ? 1u : kp == 4 ? 2u : 3u;
}
// grid of the sweeps over n rows of kp columns: 16 B per lane over n kp doubles
static inline unsigned sweep_grid(unsigned n, unsigned kp) { return lsb_k_blas1_grid(n * kp); }

#define KP_DISPATCH(kp, CALL)                                                  \
  do {                                                                         \
    switch (kshift_of(kp)) {                                                   \
    case 1: { constexpr int KP = 2; CALL; } break;                             \
    case 2: { constexpr int KP = 4; CALL; } break;                             \
    default: { constexpr int KP = 8; CALL; } break;                            \
    }                                                                          \
  } while (0)

// The launch of a CSR row kernel on blocks: g workgroups, L lanes per row (KERNEL, in parentheses, sees the count as
// the constant L), the n rows dealt in contiguous ranges that are a multiple of the WG / L rows a workgroup takes per
// trip.  The kernel's first two parameters are n and that range; the rest follow.
#define ROW_KERNEL_LAUNCH(lanes, KERNEL, g, s, n, ...)                                                                 \
  LANES_DISPATCH(lanes, (KERNEL<<<(g), WG, 0, (s)>>>((n), round_up(div_up((n), (g)), WG / L), __VA_ARGS__)))

#endif
