// gfx950 (MI355X, CDNA4) SpMV kernels of the lsbench HIP backend + their C-ABI
// launchers ("the shim").  Host code (hip_cdna4.c, plain C) never sees a
// kernel symbol, only the extern "C" lsb_k_* functions at the bottom.
//
// None of this arithmetic exists in the reference's source: every reference
// backend hands its CSR to a third-party library; the
// nearest call site is the Krylov+Jacobi apply of src/ginkgo.cpp:55-69,91-99.
// Kernel inventory = SURVEY.md section 8 (a2):
//   a2-1  spmv (adaptive row-blocked / sub-wavefront / scalar / sliced-ELL /
//         slice templates / z-columns / binned), fused p.q; the two-launch PCG
//         iteration's kernels, which walk the same z-columns
//   a2-2 .. a2-5  (dot, axpy, Jacobi, the fused PCG sweeps): hip_sweeps.hip
//
// Everything here is HBM-bandwidth bound (0.125 flop/B for a 5-point row):
// 64-wide wavefronts, coalesced 8-16 B/lane streams, LDS staging of the
// per-non-zero products, XCD-contiguous work assignment so that the x-vector
// window a row block gathers from is re-used out of one XCD's L2.  No MFMA.
#include "hip_kcommon.h"

// End of an SpMV launch with the fused dot: the workgroup's partial sum goes to
// partials[blockIdx.x]; with a tail (sharded solve over the direct xGMI path)
// the workgroup that hands in last also runs the all-reduce's contribute phase.
__device__ __forceinline__ void spmv_publish(double *__restrict__ partials, double dot,
                                             double *sred, const lsb_ar_tail &tail) {
  if (!partials)
    return;
  double d[1] = {dot};
  wg_sum<1>(d, sred);
  if (tail.counter)
    ar_tail(partials, d[0], tail);
  else if (threadIdx.x == 0)
    partials[blockIdx.x] = d[0];
}

// --------------------------------------------------------------------------
// a2-1  SpMV, adaptive row blocks.
// rowblk[k]..rowblk[k+1] is a run of consecutive rows holding <= CAP
// non-zeros, or a single row longer than CAP (lsb_csr_row_blocks).
//   * short-row block: all 256 lanes stream the block's cols/vals (fully
//     coalesced, CAP/256 loads in flight per lane), gather x, park the products
//     in LDS; then L = blklanes[k] (1..64) lanes per row add a row's products
//     and finish with a wavefront shuffle tree;
//   * long row: the whole workgroup strides over it from global memory.
// Work assignment: the row blocks are cut into 8 contiguous chunks, one per
// XCD, and inside a chunk dealt CYCLICALLY to that XCD's workgroups.  The
// G/8 workgroups resident on one XCD therefore sweep G/8 ADJACENT blocks at any
// time and the window of x they gather from (a few grid lines of a stencil)
// fits that XCD's 4 MiB L2: measured 907 -> 732 MB fetched per launch on the
// 10M-row 5-point operator (720 MB is the minimum).  A contiguous range per
// workgroup keeps 256 far-apart windows alive per XCD and thrashes it.
// SP_PREFETCH: the next block's stream loads are issued before the current
// block is reduced.  SP_NT: the once-read cols/vals stream is loaded
// nontemporal so it does not evict x from L2.  Both are picked per operator by
// a timing pass at solver creation (hip_cdna4.c).
// --------------------------------------------------------------------------
enum { SP_PREFETCH = 1, SP_NT = 2 };

template <int FLAGS, class T>
__device__ __forceinline__ T stream_load(const T *p) {
  if (FLAGS & SP_NT)
    return __builtin_nontemporal_load(p);
  return *p;
}

#define LSB_ISSUE_BLOCK(kk)                                                    \
  do {                                                                         \
    r0 = rowblk[kk], r1 = rowblk[(kk) + 1];                                    \
    j0 = offs[r0], j1 = offs[r1];                                              \
    if (j1 - j0 <= CAP) {                                                      \
      _Pragma("unroll") for (int u = 0; u < U; u++) {                          \
        const int t = (int)tid + u * WG;                                       \
        if (t < j1 - j0) {                                                     \
          c[u] = stream_load<FLAGS>(cols + j0 + t);                            \
          v[u] = stream_load<FLAGS>(vals + j0 + t);                            \
        }                                                                      \
      }                                                                        \
    }                                                                          \
  } while (0)

// VT = double, or float: opts.precision = LSB_PREC_MIXED streams the matrix
// values as fp32 (4 B instead of 8 B per entry); products and sums stay fp64.
template <int CAP, int FLAGS, class VT = double>
__global__ __launch_bounds__(WG, 8) void k_spmv_adaptive(
    const int *__restrict__ rowblk, const unsigned char *__restrict__ blklanes,
    unsigned nblk, const int *__restrict__ offs, const int *__restrict__ cols,
    const VT *__restrict__ vals, const double *__restrict__ x,
    double *__restrict__ y, const double *__restrict__ xdot,
    double *__restrict__ partials, const lsb_pcg_state *__restrict__ st,
    const int *__restrict__ rowmap, const lsb_ar_tail tail) {
  // rowmap != NULL: column-panel mode -- the CSR's rows are (row, panel) pairs,
  // row r of it accumulates into y[rowmap[r]] (one launch per panel, so a y
  // entry is touched by one lane per launch; lsb_csr_panelize)
  __shared__ double sprod[CAP];
  __shared__ double sred[4];
  const unsigned tid = threadIdx.x;
  const unsigned gx = gridDim.x / NXCD; // workgroups per XCD
  const unsigned xcd = blockIdx.x % NXCD, slot = blockIdx.x / NXCD;
  const unsigned chunk = (nblk + NXCD - 1) / NXCD; // row blocks per XCD
  const unsigned kbeg = xcd * chunk, kend = min(kbeg + chunk, nblk);
  constexpr int U = CAP / WG;
  double dot = 0.0;
  int c[U];
  VT v[U];
  int r0 = 0, r1 = 0, j0 = 0, j1 = 0;
  unsigned k = kbeg + slot;
  if (k < kend)
    LSB_ISSUE_BLOCK(k);
  // the "solve already finished" test rides behind the first block's loads
  // instead of costing a memory round trip before them
  if (st && st->status)
    return;
  for (; k < kend; k += gx) {
    const int cr0 = r0, cj0 = j0, cnt = j1 - j0, nr = r1 - r0;
    if (cnt <= CAP) {
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int t = (int)tid + u * WG;
        if (t < cnt)
          sprod[t] = (double)v[u] * x[c[u]];
      }
      if ((FLAGS & SP_PREFETCH) && k + gx < kend)
        LSB_ISSUE_BLOCK(k + gx);
      __syncthreads();
      // ---- L lanes per row add the products up -----------------------
      unsigned L;
      if (blklanes) {
        L = blklanes[k];
      } else {
        L = 1;
        while (L < 64 && (unsigned)nr * (L * 2) <= WG)
          L <<= 1;
      }
      const unsigned sl = tid / L, l = tid % L, slots = WG / L;
      for (unsigned rb = 0; rb < (unsigned)nr; rb += slots) {
        const unsigned r = rb + sl;
        double s = 0.0;
        if (r < (unsigned)nr) {
          const int a = offs[cr0 + r] - cj0, b = offs[cr0 + r + 1] - cj0;
          for (int j = a + (int)l; j < b; j += (int)L)
            s += sprod[j];
        }
        for (unsigned off = L >> 1; off > 0; off >>= 1)
          s += __shfl_xor(s, off, 64);
        if (r < (unsigned)nr && l == 0) {
          if (rowmap) {
            y[rowmap[cr0 + r]] += s;
          } else {
            y[cr0 + r] = s;
            if (xdot)
              dot += s * xdot[cr0 + r];
          }
        }
      }
      __syncthreads(); // sprod is overwritten by the next block
    } else {
      // ---- one long row (nr == 1): the whole workgroup strides over it.
      // Kept deliberately simple: an unrolled version of this rare path
      // pushed the whole kernel over 64 VGPRs into scratch and cost the
      // common path 70 % (tests/test_build_resources.py guards that).
      double s[1] = {0.0};
      for (int j = cj0 + (int)tid; j < cj0 + cnt; j += WG)
        s[0] += (double)vals[j] * x[cols[j]];
      wg_sum<1>(s, sred);
      if (tid == 0) {
        if (rowmap) {
          y[rowmap[cr0]] += s[0];
        } else {
          y[cr0] = s[0];
          if (xdot)
            dot += s[0] * xdot[cr0];
        }
      }
      if ((FLAGS & SP_PREFETCH) && k + gx < kend)
        LSB_ISSUE_BLOCK(k + gx);
    }
    if (!(FLAGS & SP_PREFETCH) && k + gx < kend)
      LSB_ISSUE_BLOCK(k + gx);
  }
  spmv_publish(partials, dot, sred, tail);
}
#undef LSB_ISSUE_BLOCK

// (Round 4, measured and taken out: k_spmv_rows -- one row per lane straight off the CSR arrays for
// operators of short rows, eight entries per trip on clamped indices, tiles of 256 rows dealt like row
// blocks; the idea: no LDS round trip, no barriers, neighbouring lanes read neighbouring 40-60 byte runs
// and re-use their lines out of L1.  10 M-row 5-point pattern with general values: 223 us (378 us with
// nontemporal stream loads, which forgo exactly that re-use) against 160 us for k_spmv_adaptive in the
// same timing pass -- a wave instruction that touches 20 lines costs the L1 more than the barriers cost
// the row-blocked form.  The CSR figure of the bench line stays k_spmv_adaptive's.)
// --------------------------------------------------------------------------
// a2-1  SpMV, L lanes per row (L = 2..64; L = 64 is the classic
// one-wavefront-per-row kernel), rows dealt to workgroups in contiguous,
// XCD-contiguous chunks; shuffle (DPP) reduction of the L partial sums.
// --------------------------------------------------------------------------
template <int L, class VT = double>
__global__ __launch_bounds__(WG) void k_spmv_subwave(
    unsigned n, unsigned rows_per_wg, const int *__restrict__ offs,
    const int *__restrict__ cols, const VT *__restrict__ vals,
    const double *__restrict__ x, double *__restrict__ y,
    const double *__restrict__ xdot, double *__restrict__ partials,
    const lsb_pcg_state *__restrict__ st) {
  __shared__ double sred[4];
  const unsigned tid = threadIdx.x, slot = tid / L, l = tid % L;
  constexpr unsigned SLOTS = WG / L;
  const unsigned w = xcd_contiguous_wg();
  const unsigned ra = min(w * rows_per_wg, n), rb = min(ra + rows_per_wg, n);
  // the status word travels with the first row's loads (this kernel serves
  // the small, latency-bound operators); nothing is stored before it is tested
  const int stopped = st ? st->status : 0;
  double dot = 0.0;
  for (unsigned base = ra; base < rb; base += SLOTS) {
    const unsigned r = base + slot;
    double s = 0.0, xd = 0.0;
    if (r < rb) {
      const int j0 = offs[r], j1 = offs[r + 1];
      if (xdot)
        xd = xdot[r];
      for (int j = j0 + (int)l; j < j1; j += L)
        s += (double)vals[j] * x[cols[j]];
    }
#pragma unroll
    for (int off = L >> 1; off > 0; off >>= 1)
      s += __shfl_xor(s, off, 64);
    if (stopped)
      return;
    if (r < rb && l == 0) {
      y[r] = s;
      dot += s * xd;
    }
  }
  if (stopped)
    return;
  if (partials) {
    double d[1] = {dot};
    wg_sum<1>(d, sred);
    if (tid == 0)
      partials[w] = d[0];
  }
}

// The launch-bound operators' iteration with the direction update folded into
// the SpMV: TWO launches per classic PCG iteration instead of three.  The
// prologue is k_pcg_update_p's (partial sums of the previous sweep -> r.z, r.r,
// stop test, beta); then q = S p_new with p_new = D^-1 r + beta p_old formed on
// the fly for every gathered column (three gathers of vectors that sit in L2)
// and stored, for the rows of this workgroup, into the OTHER direction buffer.
// At a few thousand rows a launch costs more than all of that.
template <int L>
__global__ __launch_bounds__(WG) void k_spmv_subwave_p(
    unsigned n, unsigned rows_per_wg, const int *__restrict__ offs,
    const int *__restrict__ cols, const double *__restrict__ vals,
    const double *__restrict__ r, const double *__restrict__ dinv, double dc,
    const double *__restrict__ pold, double *__restrict__ pnew, double *__restrict__ y,
    double *__restrict__ partials, lsb_pcg_state *__restrict__ st, int parity,
    const double *__restrict__ parts2, unsigned nparts2) {
  __shared__ double sred[8];
  const unsigned tid = threadIdx.x, slot = tid / L, l = tid % L;
  constexpr unsigned SLOTS = WG / L;
  const unsigned w = xcd_contiguous_wg();
  const unsigned ra = min(w * rows_per_wg, n), rb = min(ra + rows_per_wg, n);
  const int stopped = st->status;
  const double rz_old = st->rz[parity], thresh2 = st->thresh2;
  double v[2];
  wg_sum_partials<2>(parts2, nparts2, v, sred);
  if (stopped)
    return;
  const double rz_new = v[0], rr = v[1];
  const bool conv = rr <= thresh2;
  if (blockIdx.x == 0 && threadIdx.x == 0) { // exactly k_pcg_update_p's bookkeeping
    const int it = st->iters + 1;
    st->iters = it;
    st->rr = rr;
    st->rz[parity ^ 1] = rz_new;
    if (conv)
      st->status = LSB_STATUS_CONVERGED;
    else if (it >= st->maxit)
      st->status = LSB_STATUS_MAXIT;
  }
  if (conv)
    return;
  const double beta = rz_new / rz_old;
  double dot = 0.0;
  for (unsigned base = ra; base < rb; base += SLOTS) {
    const unsigned row = base + slot;
    double s = 0.0, pi = 0.0;
    if (row < rb) {
      const int j0 = offs[row], j1 = offs[row + 1];
      pi = pnew_of(dinv ? dinv[row] : dc, r[row], beta, pold[row]);
      for (int j = j0 + (int)l; j < j1; j += L) {
        const int c = cols[j];
        s += vals[j] * pnew_of(dinv ? dinv[c] : dc, r[c], beta, pold[c]);
      }
    }
#pragma unroll
    for (int off = L >> 1; off > 0; off >>= 1)
      s += __shfl_xor(s, off, 64);
    if (row < rb && l == 0) {
      pnew[row] = pi;
      y[row] = s;
      dot += s * pi;
    }
  }
  double d[1] = {dot};
  wg_sum<1>(d, sred);
  if (tid == 0)
    partials[w] = d[0];
}

// one lane per row: debug / test baseline only
__global__ __launch_bounds__(WG) void k_spmv_scalar(
    unsigned n, unsigned rows_per_wg, const int *__restrict__ offs,
    const int *__restrict__ cols, const double *__restrict__ vals,
    const double *__restrict__ x, double *__restrict__ y,
    const double *__restrict__ xdot, double *__restrict__ partials,
    const lsb_pcg_state *__restrict__ st) {
  if (st && st->status)
    return;
  __shared__ double sred[4];
  const unsigned w = xcd_contiguous_wg();
  const unsigned ra = min(w * rows_per_wg, n), rb = min(ra + rows_per_wg, n);
  double dot = 0.0;
  for (unsigned r = ra + threadIdx.x; r < rb; r += WG) {
    double s = 0.0;
    for (int j = offs[r]; j < offs[r + 1]; j++)
      s += vals[j] * x[cols[j]];
    y[r] = s;
    if (xdot)
      dot += s * xdot[r];
  }
  if (partials) {
    double d[1] = {dot};
    wg_sum<1>(d, sred);
    if (threadIdx.x == 0)
      partials[w] = d[0];
  }
}

// --------------------------------------------------------------------------
// ONE ROUNDING RULE for the sliced-ELL kernels (k_spmv_sell, k_spmv_sell16, k_spmv_tmpl): a
// row's sum is the chain a = fma(value_j, x_j, a) over its slots in slot order, written with
// explicit fma() -- not left to the compiler's contraction, which fused some products of one
// source expression and not others (slot 0 of a group in k_spmv_sell16's per-slot path came
// out as v_mul + v_add, the rest as v_fma: found when the template kernel disagreed with it in
// the last bit).  With the rule in the source every layout of one operator -- 32-bit columns,
// 16-bit codes, constant slots, templates -- produces the same bits by construction.
// --------------------------------------------------------------------------
// a2-1, sliced-ELL form (LSB_SPMV_SELL, host side lsb_csr_sellize): slices of
// 128 rows stored column-major; lane l of the slice's wavefront owns rows 2l
// and 2l+1 and reads their j-th entries as ONE int2 + ONE double2, so every
// stream instruction of a wave moves a contiguous 512 B / 1 KiB, and for a
// stencil the gathers of a wave are contiguous runs of x as well.  No LDS, no
// barrier, no row offsets; a row's products are added in column order by one
// lane (the order of a sequential CSR loop).  10 M-row 5-point: 140 us against
// 152 us for the row-blocked kernel; 64 M-row 7-point: 1.23 ms against 1.55 ms
// (tools/spmv_lab.hip).  Groups of four slices are dealt to the XCDs like the
// row blocks of k_spmv_adaptive.  [s0, s0+ns) = the slices of this launch.
// --------------------------------------------------------------------------
// Which slice does wave `wave` of this workgroup take in its turn `it`?
// period = 0: the slices [0, ns) are cut into 8 contiguous chunks, one per XCD,
// groups of four dealt cyclically to the XCD's workgroups (turns it = slot,
// slot + gx, ... < turns).  period = P > 0 (slices per plane of a 3-D stencil,
// ns a multiple of P): XCD k takes the SAME eighth [P k/8, P (k+1)/8) of every
// plane, plane after plane -- the +-plane gathers of its resident workgroups
// then stay inside ~8 of its own sections (64 M-row 7-point: 1.4 MB of x instead
// of 3.6 MB next to the matrix stream in a 4 MiB L2; PMC 5.59 -> see DESIGN.md).
// Placement is a speed matter only; every slice is taken exactly once.
struct sell_deal {
  unsigned turns, base, L, period, full, total, colturns;
};
// (Tried in round 3 and taken out: MARCHING along z -- inside its eighth of every plane a wave keeps
// ONE position and walks plane after plane, so that the +-plane operands of a step are what the
// same positions touched one and two steps ago and come out of the L2 by time rather than by the
// concurrency of the workgroups that hold the neighbouring planes.  Bit-identical, and 622-685 us
// per launch of the 64 M-row 7-point operator against 322-327 us: gpurun_out/r3_march,
// profiles/r03_cfg4_dealing.txt.)
__device__ __forceinline__ sell_deal sell_deal_init(unsigned ns, unsigned period, unsigned xcd) {
  sell_deal d;
  d.period = period, d.full = 0, d.total = 0, d.colturns = 0;
  if (!period) {
    const unsigned ngrp = (ns + 3) / 4, chunk = (ngrp + NXCD - 1) / NXCD;
    const unsigned g0 = min(xcd * chunk, ngrp), g1 = min(g0 + chunk, ngrp);
    d.base = g0 * 4, d.turns = g1 - g0, d.L = 0;
  } else {
    // whole planes first, then this XCD's part of the ragged last one (a shard
    // need not hold whole planes)
    const unsigned qlo = period * xcd / NXCD, qhi = period * (xcd + 1) / NXCD;
    const unsigned planes = ns / period, rem = ns % period;
    d.L = qhi - qlo, d.base = qlo;
    d.full = d.L * planes;
    d.total = d.full + (rem > qlo ? min(qhi, rem) - qlo : 0u);
    // z-COLUMNS: while four whole planes are left, the four waves of a workgroup take the SAME
    // position of four consecutive planes -- their +-plane operands meet in one CU at one time
    // instead of relying on other workgroups of the XCD being at the neighbouring plane just then
    // (64 M-row 7-point, k_spmv_tmpl<2>: FETCH 1166 -> 704 MB per launch for 527 MB of compulsory
    // reads; the launch time does not move, profiles/r03_cfg4_dealing.txt)
    d.colturns = (planes / 4) * d.L;
    d.turns = d.colturns + (d.total - 4 * d.colturns + 3) / 4;
  }
  return d;
}
__device__ __forceinline__ unsigned sell_deal_slice(const sell_deal &d, unsigned it, unsigned wave,
                                                    unsigned ns) {
  if (!d.period) {
    const unsigned si = d.base + it * 4 + wave;
    return si < ns ? si : 0xFFFFFFFFu;
  }
  if (it < d.colturns)
    return ((it / d.L) * 4 + wave) * d.period + d.base + it % d.L;
  const unsigned m = it * 4 + wave;
  if (m >= d.total)
    return 0xFFFFFFFFu;
  if (m < d.full)
    return (m / d.L) * d.period + d.base + m % d.L;
  return (ns / d.period) * d.period + d.base + (m - d.full);
}

typedef int i2v __attribute__((ext_vector_type(2)));
typedef int i4v __attribute__((ext_vector_type(4)));
typedef double sell_d2u __attribute__((ext_vector_type(2), aligned(8))); // a 16-byte gather at an 8-byte boundary
typedef double sell_d2v __attribute__((ext_vector_type(2)));
#define SELL_U 5
template <class VT> struct vt2;
template <> struct vt2<double> { typedef double type __attribute__((ext_vector_type(2))); };
template <> struct vt2<float> { typedef float type __attribute__((ext_vector_type(2))); };
template <int FLAGS, class VT = double>
__global__ __launch_bounds__(WG, 6) void k_spmv_sell(
    const unsigned *__restrict__ sptr, unsigned s0, unsigned ns, unsigned period, unsigned n,
    const int *__restrict__ cols, const VT *__restrict__ vals,
    const double *__restrict__ x, double *__restrict__ y, const double *__restrict__ xdot,
    double *__restrict__ partials, const lsb_pcg_state *__restrict__ st, const lsb_ar_tail tail) {
  __shared__ double sred[4];
  const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const unsigned gx = gridDim.x / NXCD, xcd = blockIdx.x % NXCD, slot = blockIdx.x / NXCD;
  const sell_deal deal = sell_deal_init(ns, period, xcd);
  const int stopped = st ? st->status : 0; // tested behind the first loads
  double dot = 0.0;
  for (unsigned g = slot; g < deal.turns; g += gx) {
    const unsigned si = __builtin_amdgcn_readfirstlane(sell_deal_slice(deal, g, wave, ns));
    if (si != 0xFFFFFFFFu) {
      const unsigned s = s0 + si;
      const unsigned base = sptr[s], len = (sptr[s + 1] - base) / LSB_SELL_ROWS;
      typedef typename vt2<VT>::type v2t;
      const i2v *cp = (const i2v *)(cols + base) + lane;
      const v2t *vp = (const v2t *)(vals + base) + lane;
      double a0 = 0.0, a1 = 0.0;
      for (unsigned j0 = 0; j0 < len; j0 += SELL_U) {
        i2v c[SELL_U];
        v2t v[SELL_U];
#pragma unroll
        for (int u = 0; u < SELL_U; u++)
          if (j0 + u < len) {
            if (FLAGS & SP_NT) {
              c[u] = __builtin_nontemporal_load(cp + (size_t)(j0 + u) * 64);
              v[u] = __builtin_nontemporal_load(vp + (size_t)(j0 + u) * 64);
            } else {
              c[u] = cp[(size_t)(j0 + u) * 64];
              v[u] = vp[(size_t)(j0 + u) * 64];
            }
          }
        if (stopped)
          return;
#pragma unroll
        for (int u = 0; u < SELL_U; u++)
          if (j0 + u < len) {
            a0 = fma((double)v[u].x, x[c[u].x], a0); // explicit: see "one rounding rule" below
            a1 = fma((double)v[u].y, x[c[u].y], a1);
          }
      }
      const unsigned row = s * LSB_SELL_ROWS + 2 * lane;
      if (row + 1 < n) {
        const sell_d2v o = {a0, a1};
        *(sell_d2v *)(y + row) = o;
        if (xdot) {
          dot = fma(a0, xdot[row], dot);
          dot = fma(a1, xdot[row + 1], dot);
        }
      } else if (row < n) {
        y[row] = a0;
        if (xdot)
          dot = fma(a0, xdot[row], dot);
      }
    }
  }
  if (stopped)
    return;
  spmv_publish(partials, dot, sred, tail);
}

// The same with 16-bit column codes (lsb_csr_sellize16): the column of the entry
// in slot j of global row g is g + base + code, {base, k} = sbase[slice, j] one
// 8-byte scalar load per slice and slot; k >= 0 says where the slot's 128 codes
// are, k = -1 that the slot has none (all its entries lie on ONE diagonal,
// folded into the base -- every slot of a structured-grid operator).  10 instead of 12 bytes per entry: 10 M-row 5-point
// 146 -> 122 us on the same box (tools/spmv_lab.hip).  A slot holds entries of
// one diagonal band, so rows can have padding BETWEEN their entries; padding
// has value 0 and is recognised by that (no gather, contributes an exact 0).
// CHEB: a Chebyshev step in the epilogue (lsb_cheb_epi, lsb_impl.h) instead of the
// store of y: the polynomial preconditioner's S z products never travel to memory.
typedef short s2v __attribute__((ext_vector_type(2)));
template <int FLAGS, class VT = double, bool CHEB = false>
__global__ __launch_bounds__(WG, 6) void k_spmv_sell16(
    const unsigned *__restrict__ sptr, unsigned s0, unsigned ns, unsigned period, unsigned n,
    unsigned row_begin, unsigned xlen, const short *__restrict__ codes, const int *__restrict__ sbase,
    const VT *__restrict__ vals, const double *__restrict__ vconst, unsigned ulen,
    const double *__restrict__ x, double *__restrict__ y, const double *__restrict__ xdot,
    double *__restrict__ partials,
    const lsb_pcg_state *__restrict__ st, const lsb_ar_tail tail, const lsb_cheb_epi epi) {
  // vconst != NULL: the constant-slot layout (lsb_sell16_value_slots) -- sbase holds
  // {base, code slot, value slot, 0} per slot, and a slot whose value slot is -1 has the
  // one value vconst[slot] for all its 128 entries (every interior diagonal of a
  // constant-coefficient stencil): 8 bytes per SLOT instead of per entry.
  __shared__ double sred[4];
  const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const unsigned gx = gridDim.x / NXCD, xcd = blockIdx.x % NXCD, slot = blockIdx.x / NXCD;
  const sell_deal deal = sell_deal_init(ns, period, xcd);
  const int stopped = st ? st->status : 0; // tested behind the first loads
  double dot = 0.0;
  for (unsigned g = slot; g < deal.turns; g += gx) {
    const unsigned si = __builtin_amdgcn_readfirstlane(sell_deal_slice(deal, g, wave, ns));
    if (si != 0xFFFFFFFFu) {
      const unsigned s = s0 + si;
      typedef typename vt2<VT>::type v2t;
      // ulen != 0: every slice has ulen slots -- no look at sptr, one memory round trip
      // less in front of the gathers (with the values gone the kernel waits on its chain
      // of dependent loads, not on bandwidth)
      const unsigned base = ulen ? s * ulen * LSB_SELL_ROWS : sptr[s];
      const unsigned len = ulen ? ulen : (sptr[s + 1] - base) / LSB_SELL_ROWS;
      const unsigned q0 = base / LSB_SELL_ROWS; // first slot of the slice
      const unsigned row = s * LSB_SELL_ROWS + 2 * lane;
      const int grow = (int)(row + row_begin);
      double a0 = 0.0, a1 = 0.0;
      sell_d2v xd = {0.0, 0.0}; // the dot's operand: asked for up front, not behind the gathers
      if (!CHEB && xdot) {
        if (row + 1 < n)
          xd = *(const sell_d2v *)(xdot + row);
        else if (row < n)
          xd.x = xdot[row];
      }
      for (unsigned j0 = 0; j0 < len; j0 += SELL_U) {
        if (vconst) {
          // The common case of a constant-coefficient operator: every slot of this group is
          // constant (no values, no padding) with one common code.  Straight-line code: all
          // slot records and constants by scalar loads in one go, then one 16-byte gather per
          // lane and slot -- rows 2l and 2l + 1 read x at grow + b and grow + b + 1 -- all in
          // flight together (a branch per slot makes every one of them a round trip of its
          // own: 61 us instead of the 3x fewer bytes' worth on the 10 M-row operator).
          const unsigned cnt = len - j0 < SELL_U ? len - j0 : SELL_U;
          i4v rec[SELL_U];
          double cst[SELL_U];
#pragma unroll
          for (int u = 0; u < SELL_U; u++) { // (past the group's end: its last slot again)
            const unsigned q = q0 + j0 + ((unsigned)u < cnt ? (unsigned)u : cnt - 1u);
            rec[u] = ((const i4v *)sbase)[q];
            cst[u] = vconst[q];
          }
          bool fast = true;
#pragma unroll
          for (int u = 0; u < SELL_U; u++)
            fast = fast && (rec[u].y < 0 && rec[u].z < 0);
          if (fast) {
            if (stopped)
              return;
            sell_d2u t[SELL_U];
#pragma unroll
            for (int u = 0; u < SELL_U; u++)
              t[u] = *(const sell_d2u *)(x + (grow + rec[u].x));
#pragma unroll
            for (int u = 0; u < SELL_U; u++)
              if ((unsigned)u < cnt) { // the same products in the same order as below
                const VT cv = (VT)cst[u];
                a0 = fma((double)cv, t[u].x, a0);
                a1 = fma((double)cv, t[u].y, a1);
              }
            continue;
          }
        }
        // Per slot: record (scalar), codes, values AND the gathers, all asked for before any of them
        // is waited for.  The gather's address does not look at the value (it used to: padding has
        // value 0 and was given address 0, which made every gather wait for its value's trip to
        // HBM): the index is clamped into x instead and the operand of a padding entry is dropped
        // at the product, an exact 0 as before.  pair: both rows of every lane gather at the same
        // offset AND the wave's 129 operands lie inside x -- one 16-byte gather per lane.
        s2v c[SELL_U];
        v2t v[SELL_U];
        sell_d2u t[SELL_U];
        const long long g0 = (long long)s * LSB_SELL_ROWS + row_begin; // global row of lane 0's first row
#pragma unroll
        for (int u = 0; u < SELL_U; u++)
          if (j0 + u < len) {
            const unsigned q = q0 + j0 + u;
            int b, kc, kv; // wave-uniform: scalar loads
            if (vconst) {
              const i4v bk = ((const i4v *)sbase)[q];
              b = bk.x, kc = bk.y, kv = bk.z;
            } else {
              const i2v bk = ((const i2v *)sbase)[q]; // {base, code slot or -1}
              b = bk.x, kc = bk.y, kv = (int)q;
            }
            c[u] = (s2v){0, 0};
            if (kc >= 0) { // slots with one common code carry none
              const s2v *cp = (const s2v *)codes + (size_t)kc * 64 + lane;
              c[u] = (FLAGS & SP_NT) ? __builtin_nontemporal_load(cp) : *cp;
            }
            if (kv >= 0) {
              const v2t *vp = (const v2t *)(vals + (size_t)kv * LSB_SELL_ROWS) + lane;
              v[u] = (FLAGS & SP_NT) ? __builtin_nontemporal_load(vp) : *vp;
            } else { // one value for the slot's 128 entries
              const VT cv = (VT)vconst[q];
              v[u] = (v2t){cv, cv};
            }
            const bool pair = kc < 0 && g0 + b >= 0 && g0 + b + (long long)LSB_SELL_ROWS <= (long long)xlen;
            if (pair) {
              t[u] = *(const sell_d2u *)(x + (grow + b));
            } else {
              long long e0 = (long long)grow + b + (int)c[u].x, e1 = (long long)grow + 1 + b + (int)c[u].y;
              e0 = e0 < 0 ? 0 : (e0 >= (long long)xlen ? (long long)xlen - 1 : e0);
              e1 = e1 < 0 ? 0 : (e1 >= (long long)xlen ? (long long)xlen - 1 : e1);
              t[u].x = x[e0], t[u].y = x[e1];
            }
          }
        if (stopped)
          return;
#pragma unroll
        for (int u = 0; u < SELL_U; u++)
          if (j0 + u < len) { // value 0 = padding: no operand, an exact 0
            a0 = fma((double)v[u].x, v[u].x != (VT)0 ? t[u].x : 0.0, a0);
            a1 = fma((double)v[u].y, v[u].y != (VT)0 ? t[u].y : 0.0, a1);
          }
      }
      if (CHEB) { // d = a d + b D^-1 (r - w); z' = z + d -- k_cheb_step's expression
        if (row + 1 < n) {
          const sell_d2v rr = *(const sell_d2v *)(epi.r + row), dd = *(const sell_d2v *)(epi.d + row);
          const double i0 = epi.dinv ? epi.dinv[row] : epi.dc, i1 = epi.dinv ? epi.dinv[row + 1] : epi.dc;
          const double v0 = fma(epi.a, dd.x, epi.b * (i0 * (rr.x - a0)));
          const double v1 = fma(epi.a, dd.y, epi.b * (i1 * (rr.y - a1)));
          const sell_d2v dn = {v0, v1}, zn = {x[grow] + v0, x[grow + 1] + v1};
          *(sell_d2v *)(epi.d + row) = dn;
          *(sell_d2v *)(epi.zout + row) = zn;
        } else if (row < n) {
          const double v0 = fma(epi.a, epi.d[row], epi.b * ((epi.dinv ? epi.dinv[row] : epi.dc) * (epi.r[row] - a0)));
          epi.d[row] = v0;
          epi.zout[row] = x[grow] + v0;
        }
      } else if (row + 1 < n) {
        const sell_d2v o = {a0, a1};
        *(sell_d2v *)(y + row) = o;
        if (xdot) {
          dot = fma(a0, xd.x, dot);
          dot = fma(a1, xd.y, dot);
        }
      } else if (row < n) {
        y[row] = a0;
        if (xdot)
          dot = fma(a0, xd.x, dot);
      }
    }
  }
  if (stopped)
    return;
  spmv_publish(partials, dot, sred, tail);
}

// --------------------------------------------------------------------------
// a2-1, sliced-ELL with slice TEMPLATES (LSB_SP_TMPL; host side lsb_sell16_templates) -- the
// constant-slot layout of a structured grid, where the shipped kernel above is bound by its
// chain of dependent loads per slice (cold slot records -> gathers), not by bytes: 176 MB in
// 41-48 us.  Measured on the 10 M-row 5-point operator (tools/stencil_lab.hip, back to back):
//   slot records by scalar loads per slice, five gathers (k_spmv_sell16)        40.8-48.0 us
//   one record per slice + the template out of the scalar cache, five gathers   32.5 us
//   + the +-1 diagonals from the centre's pair by a lane shift (three aligned
//     gathers, the dot's operand = the centre pair), straight-line              24.6-26.9 us
//   y = 4 x with the fused dot (the HBM floor of these bytes)                   23.2-24.6 us
// A wave takes a slice per turn as above.  srec[slice] (16 bytes, one scalar load) names its
// template (255: none -- the slice keeps values in a far slot or has more than 8 slots, and goes
// the per-slot way), its first kept value slot and its first mask;
// a SHAPED template is [NF far slots][c-1, c, c+1][NF far slots]: lanes gather the far slots
// and the centre c, and form the operands of c-1 / c+1 from the centre pair of the
// neighbouring lane (DPP wave shift; lane 0 and lane 63 fetch the one element beyond the
// wave's 128 by a two-lane load).  Products are formed in slot order, i.e. in the order of
// k_spmv_sell16: bit-identical results (tests/test_sell.py).
// --------------------------------------------------------------------------
__device__ __forceinline__ double lane_above(double v) { // the value lane - 1 holds (lane 0: 0)
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, 0x138, 0xf, 0xf, false); // wave_shr:1
  hi = __builtin_amdgcn_update_dpp(0, hi, 0x138, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double lane_below(double v) { // the value lane + 1 holds (lane 63: 0)
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, 0x130, 0xf, 0xf, false); // wave_shl:1
  hi = __builtin_amdgcn_update_dpp(0, hi, 0x130, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}

// values of the slots c-1 / c+1 of a shaped template where they are not plain constants.
// Masked slots (kind 2): the slice's 128-bit mask arrives in SCALAR registers (mk[side][0..1],
// loaded by the caller beside the gathers -- as two dependent vector loads behind them they
// were half of a turn's latency on the 7-point grid, where every slice holds a line end).
__device__ __forceinline__ void tmpl_side_values(const lsb_sell_tmpl *T, int NF, unsigned vb, unsigned lane,
                                                 const int (&side_k)[2], const int (&side_kd)[2],
                                                 const unsigned long long (&mk)[2][2],
                                                 const void *__restrict__ vals, int f32, double &vm0, double &vm1,
                                                 double &vp0, double &vp1) {
#pragma unroll
  for (int side = 0; side < 2; side++) {
    const int j = NF + 2 * side, k = side_k[side], kd = side_kd[side];
    if (k < 0)
      continue;
    double v0, v1;
    if (kd == 2) { // bit r of the slice's mask: row r holds the template's number
      const unsigned long long w = (lane & 32u) ? mk[side][1] : mk[side][0];
      const unsigned sh = (2u * lane) & 63u;
      v0 = (w >> sh) & 1ull ? T->cst[j] : 0.0;
      v1 = (w >> (sh + 1u)) & 1ull ? T->cst[j] : 0.0;
    } else if (f32) {
      typedef vt2<float>::type f2;
      const f2 v = *((const f2 *)((const float *)vals + (size_t)(vb + (unsigned)k) * LSB_SELL_ROWS) + lane);
      v0 = (double)v.x, v1 = (double)v.y;
    } else {
      const sell_d2v v = *((const sell_d2v *)((const double *)vals + (size_t)(vb + (unsigned)k) * LSB_SELL_ROWS) + lane);
      v0 = v.x, v1 = v.y;
    }
    if (side == 0)
      vm0 = v0, vm1 = v1;
    else
      vp0 = v0, vp1 = v1;
  }
}

typedef unsigned u4v __attribute__((ext_vector_type(4)));
#ifndef DEFER_DEPTH
#define DEFER_DEPTH 1 // turns a wave's y waits in LDS (2: 272-274 against 276-287 us on the 64 M-row 7-point operator, 29.7 against 28.2 us on the 10 M-row 5-point one)
#endif
template <int NF, bool CHEB, bool DEFER = false>
__global__ __launch_bounds__(WG, 6) void k_spmv_tmpl(
    const unsigned *__restrict__ sptr, unsigned s0, unsigned ns, unsigned period, unsigned n,
    unsigned row_begin, unsigned xlen, const u4v *__restrict__ srec,
    const unsigned long long *__restrict__ mask, const lsb_sell_tmpl *__restrict__ td,
    const int *__restrict__ sbase, const void *__restrict__ vals, int f32,
    const double *__restrict__ vconst, const double *__restrict__ x, double *__restrict__ y,
    const double *__restrict__ xdot, int dot_is_x, double *__restrict__ partials,
    const lsb_pcg_state *__restrict__ st, const lsb_ar_tail tail, const lsb_cheb_epi epi) {
  __shared__ double sred[4];
  // DEFERRED STORE.  vmcnt counts loads and stores in ONE order (gfx9), so a wave's first wait for a
  // gather also waits until the 1 KB of y it stored at the end of the turn before has been
  // acknowledged -- quick where the vectors sit in the Infinity Cache, slow where every line
  // written pushes a dirty one out to HBM (a turn of the 64 M-row 7-point operator: 4.0 us, of its
  // 50-plane slab 2.75 us; neither less traffic nor look-ahead touches changed that,
  // profiles/r03_cfg4_dealing.txt).  So a turn parks its two results per lane in LDS and the NEXT
  // turn stores them, behind its own gathers: the store is then the youngest operation in flight
  // when the gathers are waited for, and has a whole turn to complete.
  __shared__ sell_d2v ypark[DEFER ? DEFER_DEPTH * WG : 1];
  const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const unsigned gx = gridDim.x / NXCD, xcd = blockIdx.x % NXCD, slot = blockIdx.x / NXCD;
  const sell_deal deal = sell_deal_init(ns, period, xcd);
  const int stopped = st ? st->status : 0; // tested behind the first loads
  double dot = 0.0;
  // first row of the slice whose results sit in ypark[k] (wave-uniform); slot = turn % DEFER_DEPTH
  unsigned parked[DEFER_DEPTH], pslot = 0;
#pragma unroll
  for (int k = 0; k < DEFER_DEPTH; k++)
    parked[k] = 0xFFFFFFFFu;
#define TMPL_UNPARK_SLOT(K)                                                                    \
  do {                                                                                         \
    if (DEFER && parked[K] != 0xFFFFFFFFu) {                                                   \
      *(sell_d2v *)(y + parked[K] + 2 * lane) = ypark[(K) * WG + tid];                         \
      parked[K] = 0xFFFFFFFFu;                                                                 \
    }                                                                                          \
  } while (0)
#define TMPL_UNPARK()                                                                          \
  do {                                                                                         \
    if (DEFER_DEPTH == 1 || pslot == 0)                                                        \
      TMPL_UNPARK_SLOT(0);                                                                     \
    else                                                                                       \
      TMPL_UNPARK_SLOT(DEFER_DEPTH - 1);                                                       \
  } while (0)
  for (unsigned g = slot; g < deal.turns; g += gx, pslot ^= 1u) {
    const unsigned si = __builtin_amdgcn_readfirstlane(sell_deal_slice(deal, g, wave, ns));
    if (si == 0xFFFFFFFFu)
      continue;
    const unsigned s = s0 + si;
    // the slice's record {template id (255: none), first kept value slot, first mask, 0}: ONE
    // 16-byte scalar load (a byte array of ids + a pair array cost two dependent round trips, the
    // byte one through the vector path).  (Asking for it one turn ahead, beside the gathers of the
    // turn before: 320 -> 304 us on the 64 M-row 7-point operator, 25 -> 28 us on the 10 M-row
    // 5-point one whose records stay in L2; on top of the deferred store 276-287 -> 291-295 us -- not kept.)
    const u4v rec = srec[s];
    const unsigned t = __builtin_amdgcn_readfirstlane(rec.x), vb = __builtin_amdgcn_readfirstlane(rec.y);
    const unsigned mb = __builtin_amdgcn_readfirstlane(rec.z);
    const unsigned row = s * LSB_SELL_ROWS + 2 * lane;
    const int grow = (int)(row + row_begin);
    double a0 = 0.0, a1 = 0.0;
    sell_d2v xd = {0.0, 0.0};
    bool have_xd = CHEB || !xdot;
    const lsb_sell_tmpl *T = td + (t == 255u ? 0u : t);
    if (t != 255u && T->shaped) {
      const int bc = T->base[NF + 1];
      // (everything the masks' addresses need, in the same batch of scalar loads as the bases)
      const int side_k[2] = {T->kidx[NF], T->kidx[NF + 2]}, side_kd[2] = {T->kind[NF], T->kind[NF + 2]};
      sell_d2u lo[NF > 0 ? NF : 1], hi[NF > 0 ? NF : 1];
#pragma unroll
      for (int k = 0; k < NF; k++)
        lo[k] = *(const sell_d2u *)(x + (grow + T->base[k]));
      const sell_d2u c = *(const sell_d2u *)(x + (grow + bc));
#pragma unroll
      for (int k = 0; k < NF; k++)
        hi[k] = *(const sell_d2u *)(x + (grow + T->base[NF + 3 + k]));
      // the element in front of the wave's first operand of slot c-1 / behind its last of slot
      // c+1.  Where the slot is constant it exists; where it keeps values the entry it belongs to
      // may be padding at the operator's first / last row: the index is clamped (the product is
      // an exact 0 there whatever is read)
      double edge = 0.0;
      if (lane == 0 || lane == 63) {
        long long e = (long long)grow + bc + (lane == 0 ? -1 : 2);
        e = e < 0 ? 0 : (e >= (long long)xlen ? (long long)xlen - 1 : e);
        edge = x[e];
      }
      if (!have_xd && !(dot_is_x && bc == 0)) {
        if (row + 1 < n)
          xd = *(const sell_d2v *)(xdot + row);
        else if (row < n)
          xd.x = xdot[row];
        have_xd = true;
      }
      // the masks of masked slots c-1 / c+1: wave-uniform, 16 bytes each, by scalar loads that
      // travel while the gathers do
      unsigned long long mk[2][2] = {{0ull, 0ull}, {0ull, 0ull}};
#pragma unroll
      for (int side = 0; side < 2; side++)
        if (side_k[side] >= 0 && side_kd[side] == 2) {
          const unsigned long long *mp = mask + 2 * ((size_t)mb + (unsigned)side_k[side]);
          mk[side][0] = mp[0], mk[side][1] = mp[1];
        }
      TMPL_UNPARK(); // the turn before's y: behind this turn's gathers (and behind the masks' scalar
                     // loads, whose counter the LDS read shares: in front of them measured no better)
      if (stopped)
        return;
      double up = lane_above(c.y), dn = lane_below(c.x);
      if (lane == 0)
        up = edge;
      if (lane == 63)
        dn = edge;
      if (!have_xd)
        xd.x = c.x, xd.y = c.y, have_xd = true; // the centre pair IS the dot's operand
#pragma unroll
      for (int k = 0; k < NF; k++) {
        const double v = T->cst[k];
        a0 = fma(v, lo[k].x, a0), a1 = fma(v, lo[k].y, a1);
      }
      {
        // slots c-1 / c+1 may keep their values (a grid line ends inside the slice: zeros there) or
        // be MASKED: the template's number where the slice's 128-bit mask says so, else zero
        // (looked up here, behind the far slots' products: their registers are free by now)
        double vm0 = T->cst[NF], vm1 = vm0, vp0 = T->cst[NF + 2], vp1 = vp0;
        if (side_k[0] >= 0 || side_k[1] >= 0)
          tmpl_side_values(T, NF, vb, lane, side_k, side_kd, mk, vals, f32, vm0, vm1, vp0, vp1);
        // value 0 = padding: no operand, an exact 0 (the rule of k_spmv_sell16)
        const double vc = T->cst[NF + 1];
        a0 = fma(vm0, vm0 != 0.0 ? up : 0.0, a0), a1 = fma(vm1, vm1 != 0.0 ? c.x : 0.0, a1); // slot c-1: x[. - 1], x[.]
        a0 = fma(vc, c.x, a0), a1 = fma(vc, c.y, a1);                                         // slot c
        a0 = fma(vp0, vp0 != 0.0 ? c.y : 0.0, a0), a1 = fma(vp1, vp1 != 0.0 ? dn : 0.0, a1); // slot c+1
      }
#pragma unroll
      for (int k = 0; k < NF; k++) {
        const double v = T->cst[NF + 3 + k];
        a0 = fma(v, hi[k].x, a0), a1 = fma(v, hi[k].y, a1);
      }
    } else {
      TMPL_UNPARK();
      if (!have_xd) {
        if (row + 1 < n)
          xd = *(const sell_d2v *)(xdot + row);
        else if (row < n)
          xd.x = xdot[row];
        have_xd = true;
      }
      if (t != 255u) { // a pure slice of another shape (first / last grid line): every slot gathered
        const int cnt = T->nslots;
        if (stopped)
          return;
        for (int u0 = 0; u0 < LSB_TMPL_SLOTS; u0 += 4) { // (rare slices: four gathers in flight will do)
          sell_d2u v[4];
#pragma unroll
          for (int u = 0; u < 4; u++)
            if (u0 + u < cnt)
              v[u] = *(const sell_d2u *)(x + (grow + T->base[u0 + u]));
#pragma unroll
          for (int u = 0; u < 4; u++)
            if (u0 + u < cnt) {
              const double k = T->cst[u0 + u];
              a0 = fma(k, v[u].x, a0), a1 = fma(k, v[u].y, a1);
            }
        }
      } else { // a slot keeps its values (or the slice has > 8 slots): slot by slot
        const unsigned q0 = sptr[s] / LSB_SELL_ROWS, len = (sptr[s + 1] - sptr[s]) / LSB_SELL_ROWS;
        if (stopped)
          return;
        for (unsigned j = 0; j < len; j++) {
          const i4v r = ((const i4v *)sbase)[q0 + j]; // {base, -1 (no codes here), value slot or -1, 0}
          if (r.z < 0) {
            const double k = vconst[q0 + j];
            const sell_d2u v = *(const sell_d2u *)(x + (grow + r.x));
            a0 = fma(k, v.x, a0), a1 = fma(k, v.y, a1);
          } else {
            double v0, v1;
            if (f32) {
              const vt2<float>::type v = *((const vt2<float>::type *)((const float *)vals + (size_t)r.z * LSB_SELL_ROWS) + lane);
              v0 = (double)v.x, v1 = (double)v.y;
            } else {
              const sell_d2v v = *((const sell_d2v *)((const double *)vals + (size_t)r.z * LSB_SELL_ROWS) + lane);
              v0 = v.x, v1 = v.y;
            }
            const bool p0 = v0 != 0.0, p1 = v1 != 0.0; // padding: no gather, an exact 0
            const double t0 = x[p0 ? grow + r.x : 0], t1 = x[p1 ? grow + 1 + r.x : 0];
            a0 = fma(v0, p0 ? t0 : 0.0, a0), a1 = fma(v1, p1 ? t1 : 0.0, a1);
          }
        }
      }
    }
    if (CHEB) { // d = a d + b D^-1 (r - w); z' = z + d -- k_cheb_step's expression
      if (row + 1 < n) {
        const sell_d2v rr = *(const sell_d2v *)(epi.r + row), dd = *(const sell_d2v *)(epi.d + row);
        const double i0 = epi.dinv ? epi.dinv[row] : epi.dc, i1 = epi.dinv ? epi.dinv[row + 1] : epi.dc;
        const double v0 = fma(epi.a, dd.x, epi.b * (i0 * (rr.x - a0)));
        const double v1 = fma(epi.a, dd.y, epi.b * (i1 * (rr.y - a1)));
        const sell_d2v dn2 = {v0, v1}, zn = {x[grow] + v0, x[grow + 1] + v1};
        *(sell_d2v *)(epi.d + row) = dn2;
        *(sell_d2v *)(epi.zout + row) = zn;
      } else if (row < n) {
        const double v0 = fma(epi.a, epi.d[row], epi.b * ((epi.dinv ? epi.dinv[row] : epi.dc) * (epi.r[row] - a0)));
        epi.d[row] = v0;
        epi.zout[row] = x[grow] + v0;
      }
    } else if (DEFER && s * LSB_SELL_ROWS + LSB_SELL_ROWS <= n) { // a whole slice: parked, stored by the next turn
      const sell_d2v o = {a0, a1};
      if (DEFER_DEPTH == 1 || pslot == 0)
        ypark[tid] = o, parked[0] = s * LSB_SELL_ROWS;
      else
        ypark[(DEFER_DEPTH - 1) * WG + tid] = o, parked[DEFER_DEPTH - 1] = s * LSB_SELL_ROWS;
      if (xdot) {
        dot = fma(a0, xd.x, dot);
        dot = fma(a1, xd.y, dot);
      }
    } else if (row + 1 < n) {
      const sell_d2v o = {a0, a1};
      *(sell_d2v *)(y + row) = o;
      if (xdot) {
        dot = fma(a0, xd.x, dot);
        dot = fma(a1, xd.y, dot);
      }
    } else if (row < n) {
      y[row] = a0;
      if (xdot)
        dot = fma(a0, xd.x, dot);
    }
  }
#pragma unroll
  for (int k = 0; k < DEFER_DEPTH; k++)
    TMPL_UNPARK_SLOT(k);
#undef TMPL_UNPARK
#undef TMPL_UNPARK_SLOT
  if (stopped)
    return;
  spmv_publish(partials, dot, sred, tail);
}

// --------------------------------------------------------------------------
// a2-1, the template layout walked in Z-COLUMNS (LSB_SP_COL; host side lsb_sell_tmpl_columns,
// include/lsbench_hip.h).  On a 3-D stencil whose planes are whole slices the outermost far slots
// of a slice reach exactly one plane down and up, so the pair a lane gathers for slot 0 of the
// slice one plane up IS the centre pair of this slice, and this slice's last slot is that one's
// centre: a wave that walks a column s, s + period, s + 2 period, ... keeps three centre pairs in
// registers and gathers ONE new plane per step -- 3 instead of 5 gathers per 7-point slice, and
// every element of x leaves memory (K + 2) / K times instead of "three times unless the L2 still
// has it" (k_spmv_tmpl on the 64 M-row 7-point operator: FETCH 1.30 GB for 0.53 GB of compulsory
// reads).  The template, its constants and the masks of the slots c-1 / c+1 are looked at once
// per column (the host has checked that all its slices share them): a step is ~40 vector
// instructions against ~110 + ~120 scalar ones per slice of k_spmv_tmpl.
// Pipeline of a column (vmcnt counts loads and stores in one order on gfx9): a step issues the
// NEXT step's gathers, then stores the PREVIOUS step's y out of registers, then waits for its own
// operands -- which are older than both, so neither the new gathers nor the store are waited for,
// and a store has a whole step to be acknowledged (the job of LSB_SP_DEFER's LDS parking).
// Items of one slice (first / last plane, ragged ends) go slot by slot off the slot records.
// The same operands and products in the same order as k_spmv_tmpl / k_spmv_sell16: y bit for
// bit; the fused dot's partial sums follow this kernel's own (fixed) dealing.
// DOT: 0 none, 1 the centre pair is the dot's operand (xdot = x + row_begin, centre base 0), 2 loaded.
// --------------------------------------------------------------------------
template <int NF> struct col_ops { // what a step needs besides the three centre pairs
  sell_d2u lo[NF > 1 ? NF - 1 : 1], hi[NF > 1 ? NF - 1 : 1];
  double edge;
  sell_d2v xd;
};
template <int NF> struct col_tmpl { // the column's template, in scalar registers
  int bc, bl[NF > 1 ? NF - 1 : 1], bh[NF > 1 ? NF - 1 : 1];
  double k0, kl[NF > 1 ? NF - 1 : 1], kc, kh[NF > 1 ? NF - 1 : 1], kL;
};
// gu = global row of lane 0's first row in this step's slice; lrow = its local row; D = rows from a plane to the one
// ahead of it in the walk (+ a plane upward, - a plane downward)
template <int NF, int DOT>
__device__ __forceinline__ void col_issue(col_ops<NF> &o, sell_d2u &cnext, const col_tmpl<NF> &T, const double *__restrict__ x,
                                          const double *__restrict__ xdot, long long gu, unsigned lrow, long long D,
                                          unsigned xlen, unsigned lane, bool with_next) {
  if (with_next)
    cnext = *(const sell_d2u *)(x + (gu + T.bc + D) + 2 * lane);
#pragma unroll
  for (int k = 0; k < NF - 1; k++) {
    o.lo[k] = *(const sell_d2u *)(x + (gu + T.bl[k]) + 2 * lane);
    o.hi[k] = *(const sell_d2u *)(x + (gu + T.bh[k]) + 2 * lane);
  }
  // the element in front of the wave's 128 centre operands (lanes 0..31 ask for it) and the one
  // behind them (lanes 32..63): every lane loads, two addresses per wave -- no divergent branch
  // around a load, whose join would make the compiler wait for everything in flight
  // (clamped: at the operator's first / last row the slot c-1 / c+1 is masked there and whatever is
  // read is dropped at the product)
  long long el = gu + T.bc - 1, er = gu + T.bc + (long long)LSB_SELL_ROWS; // wave-uniform
  el = el < 0 ? 0 : el, er = er >= (long long)xlen ? (long long)xlen - 1 : er;
  o.edge = x[lane < 32u ? el : er];
  if (DOT == 2)
    o.xd = *(const sell_d2v *)(xdot + lrow + 2 * lane);
}
template <int NF, int DOT>
__device__ __forceinline__ void col_compute(const col_ops<NF> &o, const sell_d2u &cm, const sell_d2u &c, const sell_d2u &cp,
                                            const col_tmpl<NF> &T, double vm0, double vm1, double vp0, double vp1,
                                            unsigned lane, double &a0, double &a1, double &dot) {
  double up = lane_above(c.y), dn = lane_below(c.x);
  if (lane == 0)
    up = o.edge;
  if (lane == 63)
    dn = o.edge;
  a0 = fma(T.k0, cm.x, 0.0), a1 = fma(T.k0, cm.y, 0.0); // slot 0: one plane down = the centre of the step before
#pragma unroll
  for (int k = 0; k < NF - 1; k++)
    a0 = fma(T.kl[k], o.lo[k].x, a0), a1 = fma(T.kl[k], o.lo[k].y, a1);
  // value 0 = padding: no operand, an exact 0 (the rule of k_spmv_sell16)
  a0 = fma(vm0, vm0 != 0.0 ? up : 0.0, a0), a1 = fma(vm1, vm1 != 0.0 ? c.x : 0.0, a1); // slot c-1
  a0 = fma(T.kc, c.x, a0), a1 = fma(T.kc, c.y, a1);                                     // slot c
  a0 = fma(vp0, vp0 != 0.0 ? c.y : 0.0, a0), a1 = fma(vp1, vp1 != 0.0 ? dn : 0.0, a1); // slot c+1
#pragma unroll
  for (int k = 0; k < NF - 1; k++)
    a0 = fma(T.kh[k], o.hi[k].x, a0), a1 = fma(T.kh[k], o.hi[k].y, a1);
  a0 = fma(T.kL, cp.x, a0), a1 = fma(T.kL, cp.y, a1); // last slot: one plane up = the centre of the step after
  if (DOT == 1)
    dot = fma(a0, c.x, dot), dot = fma(a1, c.y, dot);
  else if (DOT == 2)
    dot = fma(a0, o.xd.x, dot), dot = fma(a1, o.xd.y, dot);
}

#define LSB_COL_HEAD 16 // unsigneds in front of the items: xbeg[NXCD + 1], [LSB_TMPL_COL_DOWN] the direction bits' offset
// The walk direction of a column (include/lsbench_hip.h): item `it` walks from its top slice DOWNWARD where the plan
// has direction bits and its bit is set.  A downward walk is the upward one mirrored: it starts at the column's top
// plane with the plane above it as the one "behind", and the plane ahead is the one below.  Every row's products keep
// their order -- plane below first, plane above last -- only the roles of the three registers of centre pairs turn
// round: y, q, p' and x are the same bits either way; a dot's per-lane terms come in the reverse plane order.
// The direction is wave-uniform: what a step selects between (the planes behind and ahead) is a v_cndmask per
// register, no branch.
__device__ __forceinline__ bool col_walks_down(const unsigned *__restrict__ plan, unsigned dofs, unsigned it) {
  return dofs && ((plan[dofs + (it >> 5)] >> (it & 31u)) & 1u);
}
// (a loaded dot operand is four more registers per step in flight: five workgroups per CU instead of six
// rather than spills -- the walk runs best from three or four anyway)
template <int NF, int DOT>
__global__ __launch_bounds__(WG, DOT == 2 ? 5 : 6) void k_spmv_tmpl_col(
    const unsigned *__restrict__ plan, unsigned period, unsigned n, unsigned row_begin, unsigned xlen,
    const unsigned *__restrict__ sptr, const unsigned long long *__restrict__ mask,
    const lsb_sell_tmpl *__restrict__ td, const int *__restrict__ sbase, const void *__restrict__ vals, int f32,
    const double *__restrict__ vconst, const double *__restrict__ x, double *__restrict__ y,
    const double *__restrict__ xdot, double *__restrict__ partials, const lsb_pcg_state *__restrict__ st,
    const lsb_ar_tail tail) {
  static_assert(NF >= 1 && NF <= 2, "one or two far slots per side");
  __shared__ double sred[4];
  const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const unsigned gx = gridDim.x / NXCD, xcd = blockIdx.x % NXCD, slot = blockIdx.x / NXCD;
  const unsigned i0 = plan[xcd], i1 = plan[xcd + 1];
  const u4v *__restrict__ items = (const u4v *)(plan + LSB_COL_HEAD);
  const unsigned dofs = plan[LSB_TMPL_COL_DOWN];
  const int stopped = st ? st->status : 0; // tested behind the first loads
  const unsigned P = period * LSB_SELL_ROWS; // rows of a plane
  double dot = 0.0;
  for (unsigned g = slot; i0 + 4 * g < i1; g += gx) {
    const unsigned it = __builtin_amdgcn_readfirstlane(i0 + 4 * g + wave);
    if (it >= i1)
      continue;
    const u4v rec = items[it];
    const unsigned s = __builtin_amdgcn_readfirstlane(rec.x), Kw = __builtin_amdgcn_readfirstlane(rec.y);
    const unsigned K = Kw & ~LSB_TMPL_COL_LOCKSTEP;
    // lockstep: the four items of this turn are columns of one length (the host says so in bit 31 of
    // all four): a barrier per plane keeps the workgroup's requests together
    const bool lockstep = (Kw & LSB_TMPL_COL_LOCKSTEP) != 0;
    if (K >= 2) {
      const unsigned t = __builtin_amdgcn_readfirstlane(rec.z), mb = __builtin_amdgcn_readfirstlane(rec.w);
      const lsb_sell_tmpl *T = td + t;
      col_tmpl<NF> C;
      C.bc = T->base[NF + 1];
      C.k0 = T->cst[0], C.kc = T->cst[NF + 1], C.kL = T->cst[2 * NF + 2];
#pragma unroll
      for (int k = 0; k < NF - 1; k++) {
        C.bl[k] = T->base[1 + k], C.bh[k] = T->base[NF + 3 + k];
        C.kl[k] = T->cst[1 + k], C.kh[k] = T->cst[NF + 3 + k];
      }
      const int side_k[2] = {T->kidx[NF], T->kidx[NF + 2]}, side_kd[2] = {T->kind[NF], T->kind[NF + 2]};
      // the column's masks (wave-uniform, scalar loads beside the gathers) and side values, once
      unsigned long long mk[2][2] = {{0ull, 0ull}, {0ull, 0ull}};
#pragma unroll
      for (int side = 0; side < 2; side++)
        if (side_k[side] >= 0 && side_kd[side] == 2) {
          const unsigned long long *mp = mask + 2 * ((size_t)mb + (unsigned)side_k[side]);
          mk[side][0] = mp[0], mk[side][1] = mp[1];
        }
      const bool down = col_walks_down(plan, dofs, it); // wave-uniform
      const unsigned s0 = down ? s + (K - 1) * period : s; // the plane of step 0
      const long long D = down ? -(long long)P : (long long)P;
      const unsigned Du = (unsigned)D;
      long long gu = (long long)s0 * LSB_SELL_ROWS + row_begin;
      unsigned lrow = s0 * LSB_SELL_ROWS;
      // prologue: the operands of step 0 -- the plane behind, the centre, the plane ahead
      col_ops<NF> cur, nxt;
      sell_d2u cb = *(const sell_d2u *)(x + (gu + C.bc - D) + 2 * lane);
      sell_d2u c0 = *(const sell_d2u *)(x + (gu + C.bc) + 2 * lane);
      sell_d2u ca, cn;
      col_issue<NF, DOT>(cur, ca, C, x, xdot, gu, lrow, D, xlen, lane, true);
      double vm0 = T->cst[NF], vm1 = vm0, vp0 = T->cst[NF + 2], vp1 = vp0;
      if (side_k[0] >= 0 || side_k[1] >= 0)
        tmpl_side_values(T, NF, 0u, lane, side_k, side_kd, mk, vals, f32, vm0, vm1, vp0, vp1);
      if (stopped)
        return;
      // step 0 (K >= 2: there is a next one), steps 1 .. K-2, step K-1
      col_issue<NF, DOT>(nxt, cn, C, x, xdot, gu + D, lrow + Du, D, xlen, lane, true);
      double a0, a1;
      col_compute<NF, DOT>(cur, down ? ca : cb, c0, down ? cb : ca, C, vm0, vm1, vp0, vp1, lane, a0, a1, dot);
      cb = c0, c0 = ca, ca = cn, cur = nxt;
      for (unsigned k = 1; k + 1 < K; k++) {
        gu += D, lrow += Du;
        if (lockstep)
          __builtin_amdgcn_s_barrier();
        col_issue<NF, DOT>(nxt, cn, C, x, xdot, gu + D, lrow + Du, D, xlen, lane, true);
        {
          const sell_d2v o = {a0, a1};
          *(sell_d2v *)(y + (lrow - Du) + 2 * lane) = o;
        }
        col_compute<NF, DOT>(cur, down ? ca : cb, c0, down ? cb : ca, C, vm0, vm1, vp0, vp1, lane, a0, a1, dot);
        cb = c0, c0 = ca, ca = cn, cur = nxt;
      }
      gu += D, lrow += Du;
      {
        const sell_d2v o = {a0, a1};
        *(sell_d2v *)(y + (lrow - Du) + 2 * lane) = o;
      }
      col_compute<NF, DOT>(cur, down ? ca : cb, c0, down ? cb : ca, C, vm0, vm1, vp0, vp1, lane, a0, a1, dot);
      {
        const sell_d2v o = {a0, a1};
        *(sell_d2v *)(y + lrow + 2 * lane) = o;
      }
      if (stopped)
        return;
    } else { // one slice, slot by slot off the slot records (k_spmv_tmpl's way for a slice without a template)
      const unsigned row = s * LSB_SELL_ROWS + 2 * lane;
      const int grow = (int)(row + row_begin);
      const unsigned q0 = sptr[s] / LSB_SELL_ROWS, len = (sptr[s + 1] - sptr[s]) / LSB_SELL_ROWS;
      sell_d2v xd = {0.0, 0.0};
      if (DOT) {
        if (row + 1 < n)
          xd = *(const sell_d2v *)(xdot + row);
        else if (row < n)
          xd.x = xdot[row];
      }
      if (stopped)
        return;
      double a0 = 0.0, a1 = 0.0;
      for (unsigned j = 0; j < len; j++) {
        const i4v r = ((const i4v *)sbase)[q0 + j]; // {base, -1 (no codes where templates exist), value slot or -1, 0}
        if (r.z < 0) {
          const double k = vconst[q0 + j];
          const sell_d2u v = *(const sell_d2u *)(x + (grow + r.x));
          a0 = fma(k, v.x, a0), a1 = fma(k, v.y, a1);
        } else {
          double v0, v1;
          if (f32) {
            const vt2<float>::type v = *((const vt2<float>::type *)((const float *)vals + (size_t)r.z * LSB_SELL_ROWS) + lane);
            v0 = (double)v.x, v1 = (double)v.y;
          } else {
            const sell_d2v v = *((const sell_d2v *)((const double *)vals + (size_t)r.z * LSB_SELL_ROWS) + lane);
            v0 = v.x, v1 = v.y;
          }
          const bool p0 = v0 != 0.0, p1 = v1 != 0.0; // padding: no gather, an exact 0
          const double t0 = x[p0 ? grow + r.x : 0], t1 = x[p1 ? grow + 1 + r.x : 0];
          a0 = fma(v0, p0 ? t0 : 0.0, a0), a1 = fma(v1, p1 ? t1 : 0.0, a1);
        }
      }
      if (row + 1 < n) {
        const sell_d2v o = {a0, a1};
        *(sell_d2v *)(y + row) = o;
        if (DOT)
          dot = fma(a0, xd.x, dot), dot = fma(a1, xd.y, dot);
      } else if (row < n) {
        y[row] = a0;
        if (DOT)
          dot = fma(a0, xd.x, dot);
      }
    }
  }
  if (stopped)
    return;
  spmv_publish(partials, dot, sred, tail);
}

// --------------------------------------------------------------------------
// a2-5 on a z-column plan: the classic PCG iteration in TWO launches and 60 instead of 88 bytes per
// row (one shard, constant Jacobi diagonal dc).
//   [k_pcg_col_px]   (r.z, r.r) of the sweep before -> stop test, beta;  alpha, alpha2 = the steps of the two
//                    iterations before (st->alpha[0], [1], left there by k_pcg_col_r);  per row
//                      p' = dc r + beta p        (pnew_of: k_pcg_update_p's expression)
//                      q  = S p' -- NOT stored: only the partials of p'.q leave the launch
//                      every SECOND iteration of a run (XUPD):  x += alpha2 p'' + alpha p  -- the x half of
//                        k_pcg_update_xr, two iterations' worth: p is in registers here anyway, and p'', the
//                        direction before it, is what the buffer p' goes to still holds
//                    -- reads r, p (+ x, p'') and writes p' (the OTHER direction buffer) (+ x): 24 / 48 B per row
//   [k_pcg_col_r]    alpha = r.z / p'.q;  r -= alpha (S p') with S p' formed AGAIN by the same walk (the same
//                    operands and products in the same order: the same bits);  partials of (r.z', r.r)
//                    -- reads p', r and writes r: 24 B per row
// against k_spmv_tmpl_col (16) + k_pcg_update_xr (48) + k_pcg_update_p (24): the stencil is applied twice and
// q = S p never travels.  What makes the fold pay
// where k_spmv_tmpl_p's did not (round 3: every gathered operand of every slice formed p' anew, five
// or seven times per row): a column forms p' ONCE per plane and row and keeps it in registers for the
// three steps that use it as the plane above, the centre and the plane below; only the +-line
// operands of a 3-D stencil (NF = 2) are formed a second time, out of r and p lines that sit in L2.
// Ownership: a column loads, updates and stores x and p' for ITS planes only; the plane below its
// first and above its last slice belong to other columns -- p' is formed for them, nothing stored.
// What is pending at the end of a run (one update after an even iteration, two after an odd one) has no
// k_pcg_col_px behind it: st->xpend (set by k_pcg_col_r, cleared by an updating launch here) says so and k_pcg_xfix
// applies it (hip_pcg.c).  maxit: the launch
// that counts the maxit-th iteration sets st->pad and does all of its work (x included); the next
// k_pcg_col_r turns that into the status -- never set and tested in the same launch.
// Pipeline of a column: a step issues the NEXT step's loads, waits for its own operands (older) and stores
// x, p' right away -- younger than what the next step waits for.
// --------------------------------------------------------------------------
template <int NF> struct colp_c { // centre-side loads of one step, issued ONE step ahead
  sell_d2u rn, pn;                // r, p of the plane ahead (it becomes this step's "plane above")
  sell_d2v xn, sn;                // x of that plane and the direction of TWO iterations ago (what the buffer p' goes to
                                  // still holds), where the column owns the plane and this launch updates x
  double re, pe;                  // r, p of the element in front of / behind the wave's 128 centre operands
};
// the +-line operands of a step (3-D stencil), issued TWO steps ahead: the lines a column gathers for plane z are
// the centre lines of the columns three slices to either side, which fetch them one step before they use them as
// "the plane ahead".  Asked for at that same time the request meets theirs in L2; asked for a step later (as in
// k_spmv_tmpl_col, whose steps are a quarter as long) half of them had left it again: 20.98 M fabric read requests
// per launch on the 64 M-row 7-point operator where 13 M are compulsory (profiles/r04_px.txt)
template <int NF> struct colp_m {
  sell_d2u rlo[NF > 1 ? NF - 1 : 1], plo[NF > 1 ? NF - 1 : 1], rhi[NF > 1 ? NF - 1 : 1], phi[NF > 1 ? NF - 1 : 1];
};
struct colp_out { // results of a step
  sell_d2v q, x, p;
};
// gu: global row of lane 0's first row of the step's slice (one shard: = its local row); D: rows to the plane ahead
template <int NF, bool WITH_X, int NT>
__device__ __forceinline__ void colp_issue_c(colp_c<NF> &o, const col_tmpl<NF> &T, const double *__restrict__ r,
                                             const double *__restrict__ pold, const double *__restrict__ x,
                                             const double *pstale, long long gu, long long D, unsigned xlen,
                                             unsigned lane) {
  const long long ga = gu + T.bc + D; // the plane ahead
  o.rn = *(const sell_d2u *)(r + ga + 2 * lane);
  o.pn = *(const sell_d2u *)(pold + ga + 2 * lane);
  if (WITH_X) { // x and the stale direction are touched once per launch: nontemporal (NT & 1) keeps them out of the
                // way of the r / p lines the neighbouring columns gather again
    if (NT & 1) {
      o.xn = __builtin_nontemporal_load((const sell_d2v *)(x + (gu + D) + 2 * lane));
      o.sn = __builtin_nontemporal_load((const sell_d2v *)(pstale + (gu + D) + 2 * lane));
    } else {
      o.xn = *(const sell_d2v *)(x + (gu + D) + 2 * lane);
      o.sn = *(const sell_d2v *)(pstale + (gu + D) + 2 * lane);
    }
  }
  long long el = gu + T.bc - 1, er = gu + T.bc + (long long)LSB_SELL_ROWS; // wave-uniform, clamped (see col_issue)
  el = el < 0 ? 0 : el, er = er >= (long long)xlen ? (long long)xlen - 1 : er;
  const long long e = lane < 32u ? el : er;
  o.re = r[e], o.pe = pold[e];
}
template <int NF>
__device__ __forceinline__ void colp_issue_m(colp_m<NF> &o, const col_tmpl<NF> &T, const double *__restrict__ r,
                                             const double *__restrict__ pold, long long gu, unsigned lane) {
#pragma unroll
  for (int k = 0; k < NF - 1; k++) {
    o.rlo[k] = *(const sell_d2u *)(r + (gu + T.bl[k]) + 2 * lane);
    o.plo[k] = *(const sell_d2u *)(pold + (gu + T.bl[k]) + 2 * lane);
    o.rhi[k] = *(const sell_d2u *)(r + (gu + T.bh[k]) + 2 * lane);
    o.phi[k] = *(const sell_d2u *)(pold + (gu + T.bh[k]) + 2 * lane);
  }
}
// one step: q of the centre plane from p' of the plane behind (pb), the centre (p0) and the plane ahead (pp, formed
// here) -- below, centre, above = pb, p0, pp upward (down false), pp, p0, pb downward; OWNED: the plane ahead is the
// column's own -- its x is updated and it and p' go to `out`
// XUPD: this launch applies the two pending x updates (alpha of the iteration before with its direction p, alpha2 of
// the one before that with the stale direction)
template <int NF, bool OWNED, bool XUPD>
__device__ __forceinline__ void colp_compute(const colp_c<NF> &o, const colp_m<NF> &m, const sell_d2u &pb,
                                             const sell_d2u &p0, sell_d2u &pp, bool down, const col_tmpl<NF> &T, double vm0,
                                             double vm1, double vp0, double vp1, double beta, double alpha, double alpha2,
                                             double dc, unsigned lane, colp_out &out, double &dot) {
  pp.x = pnew_of(dc, o.rn.x, beta, o.pn.x), pp.y = pnew_of(dc, o.rn.y, beta, o.pn.y);
  if (OWNED) {
    if (XUPD) { // x += alpha2 p'' + alpha p: k_pcg_update_xr's x += alpha p, two iterations' worth in their order
      out.x.x = (o.xn.x + alpha2 * o.sn.x) + alpha * o.pn.x, out.x.y = (o.xn.y + alpha2 * o.sn.y) + alpha * o.pn.y;
    }
    out.p.x = pp.x, out.p.y = pp.y;
  }
  const double edge = pnew_of(dc, o.re, beta, o.pe);
  double up = lane_above(p0.y), dn = lane_below(p0.x);
  if (lane == 0)
    up = edge;
  if (lane == 63)
    dn = edge;
  const sell_d2u &pm = down ? pp : pb, &pu = down ? pb : pp; // the planes below and above
  double a0 = fma(T.k0, pm.x, 0.0), a1 = fma(T.k0, pm.y, 0.0);
#pragma unroll
  for (int k = 0; k < NF - 1; k++) {
    const double l0 = pnew_of(dc, m.rlo[k].x, beta, m.plo[k].x), l1 = pnew_of(dc, m.rlo[k].y, beta, m.plo[k].y);
    a0 = fma(T.kl[k], l0, a0), a1 = fma(T.kl[k], l1, a1);
  }
  a0 = fma(vm0, vm0 != 0.0 ? up : 0.0, a0), a1 = fma(vm1, vm1 != 0.0 ? p0.x : 0.0, a1);
  a0 = fma(T.kc, p0.x, a0), a1 = fma(T.kc, p0.y, a1);
  a0 = fma(vp0, vp0 != 0.0 ? p0.y : 0.0, a0), a1 = fma(vp1, vp1 != 0.0 ? dn : 0.0, a1);
#pragma unroll
  for (int k = 0; k < NF - 1; k++) {
    const double h0 = pnew_of(dc, m.rhi[k].x, beta, m.phi[k].x), h1 = pnew_of(dc, m.rhi[k].y, beta, m.phi[k].y);
    a0 = fma(T.kh[k], h0, a0), a1 = fma(T.kh[k], h1, a1);
  }
  a0 = fma(T.kL, pu.x, a0), a1 = fma(T.kL, pu.y, a1);
  out.q.x = a0, out.q.y = a1;
  dot = fma(a0, p0.x, dot), dot = fma(a1, p0.y, dot);
}
// one slice, slot by slot off the slot records, every operand's p' formed on the fly (first / last
// plane, ragged ends, columns of two)
__device__ __forceinline__ void colp_single(unsigned s, unsigned n, unsigned lane, const unsigned *__restrict__ sptr,
                                            const int *__restrict__ sbase, const double *__restrict__ vals,
                                            const double *__restrict__ vconst, const double *__restrict__ r,
                                            const double *__restrict__ pold, double *pnew,
                                            double *__restrict__ x, double *__restrict__ q, double beta, double alpha,
                                            double alpha2, bool xupd, double dc, double &dot) {
  const unsigned row = s * LSB_SELL_ROWS + 2 * lane;
  const unsigned q0 = sptr[s] / LSB_SELL_ROWS, len = (sptr[s + 1] - sptr[s]) / LSB_SELL_ROWS;
  const bool l0 = row < n, l1 = row + 1 < n;
  const double r0 = l0 ? r[row] : 0.0, r1 = l1 ? r[row + 1] : 0.0;
  const double o0 = l0 ? pold[row] : 0.0, o1 = l1 ? pold[row + 1] : 0.0;
  const double x0 = xupd && l0 ? x[row] : 0.0, x1 = xupd && l1 ? x[row + 1] : 0.0;
  const double s0 = xupd && l0 ? pnew[row] : 0.0, s1 = xupd && l1 ? pnew[row + 1] : 0.0; // the direction of two iterations ago
  double a0 = 0.0, a1 = 0.0;
  for (unsigned j = 0; j < len; j++) {
    const i4v rec = ((const i4v *)sbase)[q0 + j]; // {base, -1 (no codes where templates exist), value slot or -1, 0}
    if (rec.z < 0) { // a constant slot holds 128 real entries (lsb_tmpl_check): unguarded pairs
      const double k = vconst[q0 + j];
      const sell_d2u rv = *(const sell_d2u *)(r + ((int)row + rec.x)), pv = *(const sell_d2u *)(pold + ((int)row + rec.x));
      a0 = fma(k, pnew_of(dc, rv.x, beta, pv.x), a0), a1 = fma(k, pnew_of(dc, rv.y, beta, pv.y), a1);
    } else {
      const sell_d2v v = *((const sell_d2v *)(vals + (size_t)rec.z * LSB_SELL_ROWS) + lane);
      const bool p0 = v.x != 0.0, p1 = v.y != 0.0; // padding: no gather, an exact 0
      const int c0 = p0 ? (int)row + rec.x : 0, c1 = p1 ? (int)row + 1 + rec.x : 0;
      const double t0 = pnew_of(dc, r[c0], beta, pold[c0]), t1 = pnew_of(dc, r[c1], beta, pold[c1]);
      a0 = fma(v.x, p0 ? t0 : 0.0, a0), a1 = fma(v.y, p1 ? t1 : 0.0, a1);
    }
  }
  const double n0 = pnew_of(dc, r0, beta, o0), n1 = pnew_of(dc, r1, beta, o1);
  if (l0) {
    pnew[row] = n0;
    if (xupd)
      x[row] = (x0 + alpha2 * s0) + alpha * o0;
    if (q)
      q[row] = a0;
    dot = fma(a0, n0, dot);
  }
  if (l1) {
    pnew[row + 1] = n1;
    if (xupd)
      x[row + 1] = (x1 + alpha2 * s1) + alpha * o1;
    if (q)
      q[row + 1] = a1;
    dot = fma(a1, n1, dot);
  }
}

// How the streamed results of a column leave the L2 (hip_kcommon.h: slice_store16): nothing either launch writes is
// read again in the same launch -- neighbours form p' from r and p, never from the stored p' -- so what a store leaves
// dirty in the L2 is only flushed at the launch's end, in front of the next launch's first load.  Measured on the
// 10 M-row 5-point grid (profiles/r12_col_launch_cost.txt), us per iteration: p' and x nt (the form before) 95.6-96.0,
// sc1 97.0, sc1 nt 94.3-94.5; with that, r' plain 94.3-94.5, sc1 94.1.  The same bits whatever the policy.
constexpr int COL_ST_PX = ST_SC1_NT; // k_pcg_col_px's p' and x (where NT asks for a streaming store at all)
constexpr int COL_ST_R = ST_SC1;     // k_pcg_col_r's r'
// Records of the launch before that a thread of these kernels sums with its loads in flight together
// (hip_kcommon.h: wg_sum_parts): all of a resident grid's in one batch
constexpr int COL_PARTS_U = LSB_TMPL_COL_GRID(1) / WG;
#define COLP_ST(PTR, V, BIT) slice_store16<(NT & (BIT)) ? COL_ST_PX : ST_KEEP>((PTR), lane, (V))
#define COLP_STORE(OUT, LROW, WITH_Q, WITH_XP)                                                 \
  do {                                                                                         \
    if (WITH_Q)                                                                                \
      COLP_ST(q + (LROW), (OUT).q, 2);                                                         \
    if (WITH_XP) {                                                                             \
      if (XUPD)                                                                                \
        COLP_ST(x + ((LROW) + Du), (OUT).x, 1);                                                \
      COLP_ST(pnew + ((LROW) + Du), (OUT).p, 2);                                               \
    }                                                                                          \
  } while (0)

// NT: bit 0 x loaded and stored nontemporal, bit 1 p' and q stored nontemporal
// q = S p' is NOT stored: only its dot with p' leaves the launch -- k_pcg_col_r forms the same q again out of p' when
// it updates r, and the vector never travels
// XUPD: x is updated every SECOND iteration of a run, with two directions at once -- x += alpha2 p'' + alpha p: p is
// the direction this launch reads anyway, p'' the one of the iteration before it, which is what the buffer p' goes
// to still holds (each lane reads its own rows' p'' just before it overwrites them; nobody else reads that
// buffer in this launch).  Launches of odd run index leave x alone: x is read and written half as often.
template <int NF, int NT, bool XUPD>
// (launch bounds: the resident grid of lsb_k_pcg_col_px, LSB_TMPL_COL_GRID -- three and five workgroups per CU)
__global__ __launch_bounds__(WG, NF == 2 ? 3 : 5) void k_pcg_col_px(
    const unsigned *__restrict__ plan, unsigned period, unsigned n, const unsigned *__restrict__ sptr,
    const unsigned long long *__restrict__ mask, const lsb_sell_tmpl *__restrict__ td, const int *__restrict__ sbase,
    const double *__restrict__ vals, const double *__restrict__ vconst, const double *__restrict__ r,
    const double *__restrict__ pold, double *pnew, double *__restrict__ x, double dc,
    double *__restrict__ partials, lsb_pcg_state *__restrict__ st, int parity,
    const double *__restrict__ parts2, unsigned nparts2) {
  static_assert(NF >= 1 && NF <= 2, "one or two far slots per side");
  __shared__ double sred[8];
  double *const q = nullptr; // (COLP_STORE's q leg is compiled out)
  const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const unsigned gx = gridDim.x / NXCD, xcd = blockIdx.x % NXCD, slot = blockIdx.x / NXCD;
  // ---- k_pcg_update_p's prologue: the sweep's partial sums -> r.z, r.r, stop test, beta
  const int stopped = st->status;
  const double rz_old = st->rz[parity], thresh2 = st->thresh2, alpha = st->alpha[0], alpha2 = st->alpha[1];
  const unsigned i0 = plan[xcd], i1 = plan[xcd + 1];
  double v[2];
  wg_sum_parts<2, COL_PARTS_U>(parts2, nparts2, v, sred);
  if (stopped)
    return;
  const double rz_new = v[0], rr = v[1];
  const bool conv = rr <= thresh2;
  if (blockIdx.x == 0 && threadIdx.x == 0) { // only this thread touches these words in this launch
    const int it = st->iters + 1;
    st->iters = it;
    st->rr = rr;
    st->rz[parity ^ 1] = rz_new;
    if (conv)
      st->status = LSB_STATUS_CONVERGED; // (the pending x updates stay pending: k_pcg_xfix)
    else {
      if (XUPD)
        st->xpend = 0; // this launch applies them
      if (it >= st->maxit)
        st->pad = 1; // the next k_pcg_col_r makes it the status; this launch still does all its work
    }
  }
  if (conv)
    return;
  const double beta = rz_new / rz_old;
  const u4v *__restrict__ items = (const u4v *)(plan + LSB_COL_HEAD);
  const unsigned dofs = plan[LSB_TMPL_COL_DOWN];
  const unsigned P = period * LSB_SELL_ROWS;
  double dot = 0.0;
  for (unsigned g = slot; i0 + 4 * g < i1; g += gx) {
    const unsigned it = __builtin_amdgcn_readfirstlane(i0 + 4 * g + wave);
    if (it >= i1)
      continue;
    const u4v rec = items[it];
    const unsigned s = __builtin_amdgcn_readfirstlane(rec.x);
    const unsigned K = __builtin_amdgcn_readfirstlane(rec.y) & ~LSB_TMPL_COL_LOCKSTEP;
    if (K >= 3) {
      const unsigned t = __builtin_amdgcn_readfirstlane(rec.z), mb = __builtin_amdgcn_readfirstlane(rec.w);
      const lsb_sell_tmpl *T = td + t;
      col_tmpl<NF> C;
      C.bc = T->base[NF + 1];
      C.k0 = T->cst[0], C.kc = T->cst[NF + 1], C.kL = T->cst[2 * NF + 2];
#pragma unroll
      for (int k = 0; k < NF - 1; k++) {
        C.bl[k] = T->base[1 + k], C.bh[k] = T->base[NF + 3 + k];
        C.kl[k] = T->cst[1 + k], C.kh[k] = T->cst[NF + 3 + k];
      }
      const int side_k[2] = {T->kidx[NF], T->kidx[NF + 2]}, side_kd[2] = {T->kind[NF], T->kind[NF + 2]};
      const bool down = col_walks_down(plan, dofs, it); // wave-uniform
      const unsigned s0 = down ? s + (K - 1) * period : s; // the plane of step 0
      const long long D = down ? -(long long)P : (long long)P;
      const unsigned Du = (unsigned)D;
      long long gu = (long long)s0 * LSB_SELL_ROWS;
      unsigned lrow = s0 * LSB_SELL_ROWS;
      // prologue: r, p of the plane behind (another column's) and of the first plane with its x; step 0's loads
      const long long gc = gu + C.bc;
      const sell_d2u rb = *(const sell_d2u *)(r + (gc - D) + 2 * lane);
      const sell_d2u pb = *(const sell_d2u *)(pold + (gc - D) + 2 * lane);
      const sell_d2u r0 = *(const sell_d2u *)(r + gc + 2 * lane), o0 = *(const sell_d2u *)(pold + gc + 2 * lane);
      sell_d2v x0 = {0.0, 0.0}, s0v = {0.0, 0.0};
      if (XUPD) // (a compile-time branch: no join in front of the loads)
        x0 = *(const sell_d2v *)(x + lrow + 2 * lane), s0v = *(const sell_d2v *)(pnew + lrow + 2 * lane);
      colp_c<NF> c0, c1;
      colp_m<NF> m0, m1, m2;
      colp_issue_c<NF, XUPD, NT>(c0, C, r, pold, x, pnew, gu, D, n, lane);
      colp_issue_m<NF>(m0, C, r, pold, gu, lane);
      colp_issue_m<NF>(m1, C, r, pold, gu + D, lane);
      unsigned long long mk[2][2] = {{0ull, 0ull}, {0ull, 0ull}};
#pragma unroll
      for (int side = 0; side < 2; side++)
        if (side_k[side] >= 0 && side_kd[side] == 2) {
          const unsigned long long *mp = mask + 2 * ((size_t)mb + (unsigned)side_k[side]);
          mk[side][0] = mp[0], mk[side][1] = mp[1];
        }
      double vm0 = T->cst[NF], vm1 = vm0, vp0 = T->cst[NF + 2], vp1 = vp0;
      if (side_k[0] >= 0 || side_k[1] >= 0)
        tmpl_side_values(T, NF, 0u, lane, side_k, side_kd, mk, vals, 0, vm0, vm1, vp0, vp1);
      sell_d2u pm, p0, pp; // p' of the plane behind, the centre, the plane ahead
      pm.x = pnew_of(dc, rb.x, beta, pb.x), pm.y = pnew_of(dc, rb.y, beta, pb.y);
      p0.x = pnew_of(dc, r0.x, beta, o0.x), p0.y = pnew_of(dc, r0.y, beta, o0.y);
      // A step issues the NEXT step's loads, waits for its own (older) and stores its results right away: the stores
      // are younger than the loads the next step waits for, so they are never waited for either (vmcnt counts
      // loads and stores in one order) -- no parking of results across a step.
      colp_out res;
      res.x.x = (x0.x + alpha2 * s0v.x) + alpha * o0.x, res.x.y = (x0.y + alpha2 * s0v.y) + alpha * o0.y;
      res.p.x = p0.x, res.p.y = p0.y;
      res.q = res.p; // (not stored)
      COLP_STORE(res, lrow - Du, false, true); // the first plane's x and p'
      // steps 0 .. K-3 (K >= 3): the plane after next is the column's own
      for (unsigned k = 0; k + 2 < K; k++) {
        colp_issue_c<NF, XUPD, NT>(c1, C, r, pold, x, pnew, gu + D, D, n, lane);
        colp_issue_m<NF>(m2, C, r, pold, gu + 2 * D, lane);
        colp_compute<NF, true, XUPD>(c0, m0, pm, p0, pp, down, C, vm0, vm1, vp0, vp1, beta, alpha, alpha2, dc, lane, res, dot);
        COLP_STORE(res, lrow, false, true);
        pm = p0, p0 = pp, c0 = c1, m0 = m1, m1 = m2;
        gu += D, lrow += Du;
      }
      // step K-2: the plane after next lies beyond the column's end (no x, no +-line operands to ask for)
      colp_issue_c<NF, false, NT>(c1, C, r, pold, x, pnew, gu + D, D, n, lane);
      colp_compute<NF, true, XUPD>(c0, m0, pm, p0, pp, down, C, vm0, vm1, vp0, vp1, beta, alpha, alpha2, dc, lane, res, dot);
      COLP_STORE(res, lrow, false, true);
      pm = p0, p0 = pp, c0 = c1, m0 = m1;
      gu += D, lrow += Du;
      // step K-1: nothing to load; the plane ahead is not the column's
      colp_compute<NF, false, XUPD>(c0, m0, pm, p0, pp, down, C, vm0, vm1, vp0, vp1, beta, alpha, alpha2, dc, lane, res, dot);
      COLP_STORE(res, lrow, false, false);
    } else {
      for (unsigned k = 0; k < K; k++)
        colp_single(s + k * period, n, lane, sptr, sbase, vals, vconst, r, pold, pnew, x, nullptr, beta, alpha, alpha2,
                    XUPD, dc, dot);
    }
  }
  if (partials) {
    double d[1] = {dot};
    wg_sum<1>(d, sred);
    if (threadIdx.x == 0)
      partials[blockIdx.x] = d[0];
  }
}
#undef COLP_STORE
#undef COLP_ST

// The r half of the first sweep WITHOUT q: alpha = r.z / p.q (p.q from k_pcg_col_px's partials), then per row
// r -= alpha (S p) with S p formed again by the z-column walk of k_spmv_tmpl_col -- the same operands and products in
// the same order as in k_pcg_col_px, so the same bits -- and the partials of (r.z', r.r).  Reads p and r, writes r:
// three passes, as a sweep over a stored q and r would make, but k_pcg_col_px need not write q.  Leaves alpha and "x is one update behind, the direction is in buffer pbuf" (xpend) in
// the state and promotes a pending maxit (st->pad) to the status.
template <int NF>
__global__ __launch_bounds__(WG, 5) void k_pcg_col_r(
    const unsigned *__restrict__ plan, unsigned period, unsigned n, const unsigned *__restrict__ sptr,
    const unsigned long long *__restrict__ mask, const lsb_sell_tmpl *__restrict__ td, const int *__restrict__ sbase,
    const double *__restrict__ vals, const double *__restrict__ vconst, const double *__restrict__ p,
    double *__restrict__ r, double dc, lsb_pcg_state *__restrict__ st, int parity, int pbuf, int xtwo, int rev,
    const double *__restrict__ pq_parts, unsigned npq, double *__restrict__ partials2) {
  static_assert(NF >= 1 && NF <= 2, "one or two far slots per side");
  __shared__ double sred[8];
  const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const unsigned gx = gridDim.x / NXCD, xcd = blockIdx.x % NXCD, slot = blockIdx.x / NXCD;
  const int stopped = st->status, pad = st->pad;
  const double rz = st->rz[parity];
  const unsigned i0 = plan[xcd], i1 = plan[xcd + 1];
  double pqv[1];
  wg_sum_parts<1, COL_PARTS_U>(pq_parts, npq, pqv, sred);
  if (stopped)
    return;
  if (pad) { // the launch before counted the maxit-th iteration (and did its x update): stop here
    if (blockIdx.x == 0 && threadIdx.x == 0)
      st->status = LSB_STATUS_MAXIT;
    return;
  }
  const double pq = pqv[0];
  if (!(pq != 0.0) || !isfinite(pq)) { // same decision in every workgroup
    if (blockIdx.x == 0 && threadIdx.x == 0)
      st->status = LSB_STATUS_BREAKDOWN;
    return;
  }
  const double alpha = rz / pq;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    // x is now one update behind (the run's even iterations: k_pcg_col_px has just applied the two before) or two
    // (odd ones: the launch before left x alone): xpend = 1 + pbuf / 3 + pbuf, the steps in alpha[0] and alpha[1]
    st->pq = pq, st->alpha[1] = st->alpha[0], st->alpha[0] = alpha, st->xpend = (xtwo ? 3 : 1) + pbuf;
  }
  const u4v *__restrict__ items = (const u4v *)(plan + LSB_COL_HEAD);
  const unsigned dofs = plan[LSB_TMPL_COL_DOWN];
  const unsigned P = period * LSB_SELL_ROWS;
  double acc[2] = {0.0, 0.0}, nodot = 0.0;
#define COLR_FINISH(A0, A1, RV, LROW)                                                          \
  do {                                                                                         \
    sell_d2v rn_;                                                                              \
    rn_.x = (RV).x - alpha * (A0), rn_.y = (RV).y - alpha * (A1);                              \
    slice_store16<COL_ST_R>(r + (LROW), lane, rn_);                                            \
    acc[0] += rn_.x * (dc * rn_.x);                                                            \
    acc[0] += rn_.y * (dc * rn_.y);                                                            \
    acc[1] += rn_.x * rn_.x;                                                                   \
    acc[1] += rn_.y * rn_.y;                                                                   \
  } while (0)
  // rev: the turns take the band's groups of four from its END -- the launch before (k_pcg_col_px, ascending) touched
  // those lines last, so this one starts on what is still in the Infinity Cache and the next ascending launch in turn
  // starts where this one ended.  The groups, their lockstep bits and walk directions are the plan's either way; every
  // row's r' is the same bits, only the order in which a thread adds its terms of (r.z', r.r) follows the turns.
  const unsigned G = (i1 - i0 + 3u) / 4u;
  for (unsigned j = slot; j < G; j += gx) {
    const unsigned g = rev ? G - 1u - j : j;
    const unsigned it = __builtin_amdgcn_readfirstlane(i0 + 4 * g + wave);
    if (it >= i1)
      continue;
    const u4v rec = items[it];
    const unsigned s = __builtin_amdgcn_readfirstlane(rec.x);
    const unsigned K = __builtin_amdgcn_readfirstlane(rec.y) & ~LSB_TMPL_COL_LOCKSTEP;
    if (K >= 3) { // (columns of two go slice by slice, as in k_pcg_col_px: the same sums either way)
      const unsigned t = __builtin_amdgcn_readfirstlane(rec.z), mb = __builtin_amdgcn_readfirstlane(rec.w);
      const lsb_sell_tmpl *T = td + t;
      col_tmpl<NF> C;
      C.bc = T->base[NF + 1];
      C.k0 = T->cst[0], C.kc = T->cst[NF + 1], C.kL = T->cst[2 * NF + 2];
#pragma unroll
      for (int k = 0; k < NF - 1; k++) {
        C.bl[k] = T->base[1 + k], C.bh[k] = T->base[NF + 3 + k];
        C.kl[k] = T->cst[1 + k], C.kh[k] = T->cst[NF + 3 + k];
      }
      const int side_k[2] = {T->kidx[NF], T->kidx[NF + 2]}, side_kd[2] = {T->kind[NF], T->kind[NF + 2]};
      const bool down = col_walks_down(plan, dofs, it); // wave-uniform
      const unsigned s0 = down ? s + (K - 1) * period : s; // the plane of step 0
      const long long D = down ? -(long long)P : (long long)P;
      const unsigned Du = (unsigned)D;
      long long gu = (long long)s0 * LSB_SELL_ROWS;
      unsigned lrow = s0 * LSB_SELL_ROWS;
      col_ops<NF> cur, nxt;
      sell_d2u cb = *(const sell_d2u *)(p + (gu + C.bc - D) + 2 * lane);
      sell_d2u c0 = *(const sell_d2u *)(p + (gu + C.bc) + 2 * lane);
      sell_d2u ca, cn;
      col_issue<NF, 2>(cur, ca, C, p, r, gu, lrow, D, n, lane, true); // (the "dot operand" slot carries r's pair)
      unsigned long long mk[2][2] = {{0ull, 0ull}, {0ull, 0ull}};
#pragma unroll
      for (int side = 0; side < 2; side++)
        if (side_k[side] >= 0 && side_kd[side] == 2) {
          const unsigned long long *mp = mask + 2 * ((size_t)mb + (unsigned)side_k[side]);
          mk[side][0] = mp[0], mk[side][1] = mp[1];
        }
      double vm0 = T->cst[NF], vm1 = vm0, vp0 = T->cst[NF + 2], vp1 = vp0;
      if (side_k[0] >= 0 || side_k[1] >= 0)
        tmpl_side_values(T, NF, 0u, lane, side_k, side_kd, mk, vals, 0, vm0, vm1, vp0, vp1);
      for (unsigned k = 0; k + 1 < K; k++) {
        col_issue<NF, 2>(nxt, cn, C, p, r, gu + D, lrow + Du, D, n, lane, true);
        double a0, a1;
        col_compute<NF, 0>(cur, down ? ca : cb, c0, down ? cb : ca, C, vm0, vm1, vp0, vp1, lane, a0, a1, nodot);
        COLR_FINISH(a0, a1, cur.xd, lrow);
        cb = c0, c0 = ca, ca = cn, cur = nxt;
        gu += D, lrow += Du;
      }
      double a0, a1;
      col_compute<NF, 0>(cur, down ? ca : cb, c0, down ? cb : ca, C, vm0, vm1, vp0, vp1, lane, a0, a1, nodot);
      COLR_FINISH(a0, a1, cur.xd, lrow);
    } else {
      for (unsigned k = 0; k < K; k++) { // one slice, slot by slot off the slot records
        const unsigned sl = s + k * period, row = sl * LSB_SELL_ROWS + 2 * lane;
        const unsigned q0 = sptr[sl] / LSB_SELL_ROWS, len = (sptr[sl + 1] - sptr[sl]) / LSB_SELL_ROWS;
        const bool l0 = row < n, l1 = row + 1 < n;
        const double r0 = l0 ? r[row] : 0.0, r1 = l1 ? r[row + 1] : 0.0;
        double a0 = 0.0, a1 = 0.0;
        for (unsigned j = 0; j < len; j++) {
          const i4v rec2 = ((const i4v *)sbase)[q0 + j];
          if (rec2.z < 0) {
            const double kk = vconst[q0 + j];
            const sell_d2u pv = *(const sell_d2u *)(p + ((int)row + rec2.x));
            a0 = fma(kk, pv.x, a0), a1 = fma(kk, pv.y, a1);
          } else {
            const sell_d2v v = *((const sell_d2v *)(vals + (size_t)rec2.z * LSB_SELL_ROWS) + lane);
            const bool p0 = v.x != 0.0, p1 = v.y != 0.0; // padding: no gather, an exact 0
            const double t0 = p[p0 ? (int)row + rec2.x : 0], t1 = p[p1 ? (int)row + 1 + rec2.x : 0];
            a0 = fma(v.x, p0 ? t0 : 0.0, a0), a1 = fma(v.y, p1 ? t1 : 0.0, a1);
          }
        }
        if (l0) {
          const double rn0 = r0 - alpha * a0;
          r[row] = rn0;
          acc[0] += rn0 * (dc * rn0), acc[1] += rn0 * rn0;
        }
        if (l1) {
          const double rn1 = r1 - alpha * a1;
          r[row + 1] = rn1;
          acc[0] += rn1 * (dc * rn1), acc[1] += rn1 * rn1;
        }
      }
    }
  }
#undef COLR_FINISH
  wg_sum<2>(acc, sred);
  if (threadIdx.x == 0) {
    partials2[2 * blockIdx.x + 0] = acc[0];
    partials2[2 * blockIdx.x + 1] = acc[1];
  }
}


// (Round 4, measured and taken out again: k_spmv_tmpl_deep -- a wave takes 2 or 4 of its turns AT ONCE,
// all their slice records in one batch of scalar loads, all 10 / 20 gathers, edge elements and mask
// words in flight together, the stores of the group before behind them; 90 / 136 VGPRs, 5 / 3 waves per
// SIMD, 40 / 48 slices in flight per CU instead of 24; bit-identical, fused dot included.  64 M-row
// 7-point operator, same box: 332 / 336 us back to back against 302 us for the deferred-store form
// below and 345 us for the plain one; 10 M-row 5-point: 28.3 / 32.5 against 25.9 us.  So the launch
// is NOT short of bytes in flight -- round 3's reading -- and the counters agree: its fabric reads wait
// 1200-1450 L2 cycles where the sweeps' wait 2300-2700 at 1.4-2x the requests outstanding.  What a
// slice costs is mostly there when everything sits in the Infinity Cache too (0.45 of 0.60 ns per
// slice): ~110 vector and ~120 scalar instructions per slice and wave, five L1->L2 round trips of
// which three hit L2.  profiles/r04_cfg4_spmv.txt; the kernel is in the history
// at commit "Vectors of a shard carved out of one allocation".)
// --------------------------------------------------------------------------
// a2-1, binned form (LSB_SPMV_BINNED, host side lsb_csr_binize) -- for operators
// whose rows scatter over far more of x than an XCD's L2 holds (power-law
// config 5: PMC shows 2.7e8 L2 misses per launch of the row-major kernel, one
// 128-byte line per non-zero, 34 GB of fabric traffic for 3.2 GB of algorithmic
// bytes).  One launch per BIN = per 2 MiB window of x, so every gather of the
// launch hits L2 after first touch; inside the bin the entries come as a
// row-sorted (row, col, value) stream and are cut into chunks of whole rows.
// A workgroup takes one chunk:
//   1. all 256 lanes stream 8 entries each (coalesced), gather x, and park
//      product and row id in LDS;
//   2. lane t then owns the 8 CONSECUTIVE entries [8t, 8t+8): it adds up the
//      runs of equal row ids in them -- a run that begins and ends inside is
//      added to y at once -- and what is left open at either end goes through
//      a segmented scan over the lanes (wavefront shuffles, then the four
//      waves through LDS);
//   3. the lane in which a multi-lane run ends adds carry + its own part to y.
// Every lane does the same amount of work whatever the row lengths are (the
// row-blocked kernel's reduce phase serialises on a block's longest row), each
// y entry is touched by exactly one lane per launch (no atomics), and the order
// of the additions is fixed by the layout alone: bit-identical run to run.
// --------------------------------------------------------------------------
__device__ __forceinline__ unsigned bin_pad(unsigned i) { return i + (i >> 3); }

template <int FLAGS, int BIN_U>
__global__ __launch_bounds__(WG) void k_spmv_binned(
    const unsigned *__restrict__ chunk_begin, unsigned nchunk, const unsigned *__restrict__ rows,
    const unsigned *__restrict__ cols, const double *__restrict__ vals,
    const double *__restrict__ x, double *__restrict__ y, const lsb_pcg_state *__restrict__ st) {
  constexpr unsigned CHUNK = BIN_U * WG; // entries of a chunk: 1024, 1536 or 2048
  __shared__ double sprod[CHUNK + CHUNK / 8 + 8];
  __shared__ unsigned skey[CHUNK + CHUNK / 8 + 8];
  __shared__ double swv[4];
  __shared__ int swf[4];
  __shared__ double sred[4];
  const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  // XCD-contiguous chunk ids: an XCD's workgroups sweep neighbouring rows of y
  const unsigned per = gridDim.x / NXCD;
  const unsigned w = (blockIdx.x % NXCD) * per + blockIdx.x / NXCD;
  if (w >= nchunk)
    return;
  const unsigned e0 = chunk_begin[w], cnt = chunk_begin[w + 1] - e0;
  unsigned r[BIN_U], c[BIN_U];
  double v[BIN_U];
  if (cnt <= CHUNK) {
#pragma unroll
    for (int u = 0; u < BIN_U; u++) {
      const unsigned t = tid + u * WG;
      if (t < cnt) {
        r[u] = stream_load<FLAGS>(rows + e0 + t);
        c[u] = stream_load<FLAGS>(cols + e0 + t);
        v[u] = stream_load<FLAGS>(vals + e0 + t);
      }
    }
  }
  if (st && st->status)
    return;
  if (cnt > CHUNK) { // ONE run longer than a chunk: the workgroup strides over it
    double s[1] = {0.0};
    for (unsigned j = e0 + tid; j < e0 + cnt; j += WG)
      s[0] += vals[j] * x[cols[j]];
    wg_sum<1>(s, sred);
    if (tid == 0)
      y[rows[e0]] += s[0];
    return;
  }
#pragma unroll
  for (int u = 0; u < BIN_U; u++) {
    const unsigned t = tid + u * WG;
    if (t < cnt) {
      // how the window of x is gathered out of L2 is a tuning flag: plain loads
      // fill a 128-byte L1 line per gather for 8 bytes used
      double xv;
      if (FLAGS & 8)
        xv = __hip_atomic_load(x + c[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else if (FLAGS & 16)
        xv = __builtin_nontemporal_load(x + c[u]);
      else
        xv = x[c[u]];
      sprod[bin_pad(t)] = v[u] * xv;
      skey[bin_pad(t)] = r[u];
    }
  }
  __syncthreads();
  // ---- lane t: entries [8t, 8t+8) -------------------------------------------
  const unsigned i0 = tid * BIN_U;
  const int nloc = i0 < cnt ? (int)min(cnt - i0, (unsigned)BIN_U) : 0;
  double first_sum = 0.0, acc = 0.0;
  unsigned first_key = 0, prevk = 0xFFFFFFFFu, nextk = 0xFFFFFFFEu;
  bool cont = false, has_boundary = false, closes = true;
  // runs that END inside this lane and did not begin in an earlier one are added
  // to y by this lane alone: collect them first, then ALL the loads of y, then
  // the stores -- a load-add-store chain per run would serialise up to eight
  // memory round trips per lane (short rows: nearly every entry ends a run)
  unsigned ok_[BIN_U];
  double ov[BIN_U];
  unsigned omask = 0;
  if (nloc > 0) {
    if (i0 > 0)
      prevk = skey[bin_pad(i0 - 1)];
    if (i0 + BIN_U < cnt)
      nextk = skey[bin_pad(i0 + BIN_U)];
    unsigned k[BIN_U + 1];
    double p[BIN_U];
#pragma unroll
    for (int j = 0; j < BIN_U; j++) {
      k[j] = j < nloc ? skey[bin_pad(i0 + j)] : 0u;
      p[j] = j < nloc ? sprod[bin_pad(i0 + j)] : 0.0;
    }
    cont = k[0] == prevk;
    first_key = k[0];
#pragma unroll
    for (int j = 0; j < BIN_U; j++)
      if (j < nloc) {
        acc += p[j];
        const bool last = j == nloc - 1;
        const bool ends = last ? (k[j] != nextk) : (k[j + 1] != k[j]);
        if (last)
          closes = ends;
        if (ends) {
          if (cont && !has_boundary) {
            first_sum = acc; // the head run: needs the carry of the lanes before
          } else {
            omask |= 1u << j;
            ok_[j] = k[j], ov[j] = acc;
          }
          if (!last)
            has_boundary = true, acc = 0.0;
        }
      }
    // (has_boundary = a run begins after this lane's first entry)
    double yv[BIN_U];
#pragma unroll
    for (int j = 0; j < BIN_U; j++)
      if (omask & (1u << j))
        yv[j] = y[ok_[j]];
#pragma unroll
    for (int j = 0; j < BIN_U; j++)
      if (omask & (1u << j))
        y[ok_[j]] = yv[j] + ov[j];
  }
  // ---- what is open at the lane ends: segmented scan over the lanes --------
  // value = sum of the lane's last run, flag = "a run begins in this lane"
  double sv = acc;
  int sf = (has_boundary || !cont) ? 1 : 0;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double v2 = __shfl_up(sv, d, 64);
    const int f2 = __shfl_up(sf, d, 64);
    if ((int)lane >= d) {
      if (!sf)
        sv += v2;
      sf |= f2;
    }
  }
  if (lane == 63)
    swv[wave] = sv, swf[wave] = sf;
  __syncthreads();
  double carry_w = 0.0;
  for (unsigned q = 0; q < wave; q++)
    carry_w = swf[q] ? swv[q] : carry_w + swv[q];
  const double incl = sv + (sf ? 0.0 : carry_w); // sum of the open run up to and including this lane
  double carry_in = __shfl_up(incl, 1, 64);
  if (lane == 0)
    carry_in = carry_w;
  // the head run of a lane that continues a run of the lanes before, where it ends
  // in this lane (inside it, or with its last entry)
  if (nloc > 0 && cont && (has_boundary || closes))
    y[first_key] += carry_in + first_sum;
}

// (C linkage admits no templates: the launchers' pick of a binned kernel by its chunk size lives out here)
template <int FLAGS> static decltype(&k_spmv_binned<0, 4>) binned_kern(unsigned chunk_cap) {
  return chunk_cap == 1024 ? k_spmv_binned<FLAGS, 4> : chunk_cap == 1536 ? k_spmv_binned<FLAGS, 6> : k_spmv_binned<FLAGS, 8>;
}

extern "C" {

/* one bin of the binned form: chunks [c0, c0 + nchunk) */
void lsb_k_spmv_binned(unsigned flags, unsigned chunk_cap, const unsigned *chunk_begin, unsigned c0,
                       unsigned nchunk, const unsigned *rows, const unsigned *cols, const double *vals,
                       const double *x, double *y, const struct lsb_pcg_state *st, void *stream) {
  if (!nchunk)
    return;
  const unsigned g = (nchunk + NXCD - 1) / NXCD * NXCD;
  auto kern = k_spmv_binned<SP_NT, 8>;
  switch (flags & (SP_NT | 8u | 16u)) {
  case 0: kern = binned_kern<0>(chunk_cap); break;
  case 2: kern = binned_kern<2>(chunk_cap); break;
  case 8: kern = binned_kern<8>(chunk_cap); break;
  case 10: kern = binned_kern<10>(chunk_cap); break;
  case 16: kern = binned_kern<16>(chunk_cap); break;
  case 18: kern = binned_kern<18>(chunk_cap); break;
  }
  kern<<<g, WG, 0, (hipStream_t)stream>>>(chunk_begin + c0, nchunk, rows, cols, vals, x, y, st);
}

// number of workgroups (== number of dot partials) a given SpMV launch uses
unsigned lsb_k_spmv_grid(int variant, unsigned n, unsigned nblk,
                         unsigned lanes_per_row, unsigned grid_cap) {
  unsigned items;
  if (variant == LSB_SPMV_SELL) /* four slices per workgroup step */
    items = div_up(nblk, 4);
  else if (variant == LSB_SPMV_ADAPTIVE)
    items = nblk;
  else if (variant == LSB_SPMV_SUBWAVE)
    items = div_up(n, WG / (lanes_per_row ? lanes_per_row : 1));
  else
    items = div_up(n, WG);
  unsigned g = round_up(items ? items : 1, NXCD);
  if (grid_cap == 0 || grid_cap > LSB_MAX_PARTIALS)
    grid_cap = LSB_MAX_PARTIALS;
  grid_cap = grid_cap / NXCD * NXCD;
  if (grid_cap < NXCD)
    grid_cap = NXCD;
  if (g > grid_cap) {
    g = grid_cap;
    /* The persistent kernels cut the items into NXCD chunks and deal a chunk
     * cyclically to the XCD's g/NXCD workgroups: size the grid so that every
     * workgroup gets the same number of items (2440 items on 1536 workgroups
     * is two rounds with the second 59 % full; on 1224 it is two full ones,
     * and the consumers re-reduce 1224 partial sums instead of 1536). */
    if (variant == LSB_SPMV_SELL || variant == LSB_SPMV_ADAPTIVE) {
      const unsigned chunk = div_up(items, NXCD), cap = grid_cap / NXCD;
      const unsigned per = div_up(chunk, cap);
      g = div_up(chunk, per) * NXCD;
    }
  }
  return g;
}

/* the kernels with spmv_publish at their end */
int lsb_k_spmv_has_tail(int variant) { return variant == LSB_SPMV_ADAPTIVE || variant == LSB_SPMV_SELL; }

static lsb_ar_tail tail_for(const struct lsb_ar_tail *t, const double *partials) {
  lsb_ar_tail none;
  memset(&none, 0, sizeof none);
  if (!t || !t->counter)
    return none;
  if (!partials)
    errx(EXIT_FAILURE, "an SpMV launch without dot partials cannot carry the all-reduce");
  return *t;
}

static lsb_cheb_epi epi_for(const struct lsb_cheb_epi *e, bool refused, const char *why) {
  lsb_cheb_epi none;
  memset(&none, 0, sizeof none);
  if (!e || !e->zout)
    return none;
  if (refused)
    errx(EXIT_FAILURE, "%s", why);
  return *e;
}

void lsb_k_spmv(int variant, unsigned n, const int *offs, const int *cols,
                const double *vals, const int *rowblk,
                const unsigned char *blklanes, unsigned nblk,
                unsigned lanes_per_row, unsigned flags, unsigned grid_cap,
                const double *x, double *y, const double *xdot,
                double *partials, unsigned *npartials,
                const struct lsb_pcg_state *st, const int *rowmap,
                const struct lsb_ar_tail *tail_in, void *stream) {
  /* flags & LSB_SP_F32: `vals` points at fp32 values (mixed precision) */
  hipStream_t s = (hipStream_t)stream;
  const lsb_ar_tail tail = tail_for(tail_in, partials);
  if (tail.counter && !lsb_k_spmv_has_tail(variant))
    errx(EXIT_FAILURE, "lsb_k_spmv: SpMV form %d cannot carry the all-reduce", variant);
  const unsigned g = lsb_k_spmv_grid(variant, n, nblk, lanes_per_row, grid_cap);
  if (npartials)
    *npartials = g;
  auto launch = [&](auto *v) { /* v: the values, of the kernel's value type */
    using VT = std::decay_t<decltype(*v)>;
    if (variant == LSB_SPMV_ADAPTIVE) {
      static decltype(&k_spmv_adaptive<LSB_BLOCK_NNZ, 0, VT>) const kern[4] = { /* [flags & 3] */
          k_spmv_adaptive<LSB_BLOCK_NNZ, 0, VT>, k_spmv_adaptive<LSB_BLOCK_NNZ, 1, VT>,
          k_spmv_adaptive<LSB_BLOCK_NNZ, 2, VT>, k_spmv_adaptive<LSB_BLOCK_NNZ, 3, VT>};
      kern[flags & 3u]<<<g, WG, 0, s>>>(rowblk, blklanes, nblk, offs, cols, v, x, y, xdot, partials, st, rowmap, tail);
    } else {
      LANES_DISPATCH(lanes_per_row, (k_spmv_subwave<L, VT><<<g, WG, 0, s>>>(n, round_up(div_up(n, g), WG / L), offs, cols,
                                                                           v, x, y, xdot, partials, st)));
    }
  };
  if (variant != LSB_SPMV_ADAPTIVE && variant != LSB_SPMV_SUBWAVE)
    k_spmv_scalar<<<g, WG, 0, s>>>(n, div_up(n, g), offs, cols, vals, x, y, xdot, partials, st);
  else if (flags & LSB_SP_F32)
    launch((const float *)(const void *)vals);
  else
    launch(vals);
}

/* sub-wavefront SpMV with the direction update of the previous iteration folded
 * in (k_spmv_subwave_p); same grid as the plain sub-wavefront launch */
void lsb_k_spmv_subwave_p(unsigned n, const int *offs, const int *cols, const double *vals,
                          unsigned lanes_per_row, const double *r, const double *dinv, double dc,
                          const double *pold, double *pnew, double *y, double *partials,
                          unsigned *npartials, struct lsb_pcg_state *st, int parity,
                          const double *parts2, unsigned nparts2, void *stream) {
  const unsigned g = lsb_k_spmv_grid(LSB_SPMV_SUBWAVE, n, 0, lanes_per_row, 0);
  *npartials = g;
  LANES_DISPATCH(lanes_per_row, (k_spmv_subwave_p<L><<<g, WG, 0, (hipStream_t)stream>>>(
                                    n, round_up(div_up(n, g), WG / L), offs, cols, vals, r, dinv, dc, pold, pnew, y,
                                    partials, st, parity, parts2, nparts2)));
}

/* What the sliced-ELL, template and z-column launchers share, over `items` slices or column items: the
 * all-reduce tail; the grid -- grid_cap, LSB_SELL_GRID where that is 0, at most `resident` where that is
 * given -- and *npartials; the period (a slice launch deals its slices contiguously where the period is
 * less than a plane, a column launch keeps its plan's); the far slots per side of c's templates (0 .. 2,
 * a column launch 1 .. 2; c == NULL: no templates). */
struct sell_launch {
  unsigned g, period;
  lsb_ar_tail tail;
};
static sell_launch sell_prologue(const char *who, bool col, const struct lsb_sell16_dev *c, unsigned items,
                                 unsigned n, unsigned grid_cap, unsigned resident, unsigned period,
                                 const double *partials, unsigned *npartials, const struct lsb_ar_tail *tail_in) {
  sell_launch L;
  L.tail = tail_for(tail_in, partials);
  unsigned cap = grid_cap ? grid_cap : resident ? resident : LSB_SELL_GRID;
  if (resident && cap > resident)
    cap = resident;
  L.g = lsb_k_spmv_grid(LSB_SPMV_SELL, n, items, 0, cap);
  if (npartials)
    *npartials = L.g;
  L.period = !col && period && (period < NXCD || items < period) ? 0 : period;
  if (c && (c->tmpl.nfar > 2 || (col && c->tmpl.nfar < 1)))
    errx(EXIT_FAILURE, "%s: %u far slots per side", who, c->tmpl.nfar);
  return L;
}

/* Sliced-ELL launch over the slices [s0, s0+ns).  flags & LSB_SP_C16: `cols` is
 * the 16-bit code array and `sbase` the slot bases (row_begin = global index
 * of local row 0); else `cols` holds 32-bit column ids and sbase is unused. */
void lsb_k_spmv_sell(unsigned flags, unsigned grid_cap, unsigned period, const unsigned *sptr,
                     unsigned s0, unsigned ns, unsigned n, unsigned row_begin, unsigned xlen,
                     const void *cols,
                     const int *sbase, const double *vals, const double *vconst, unsigned ulen,
                     const double *x, double *y, const double *xdot, double *partials,
                     unsigned *npartials,
                     const struct lsb_pcg_state *st, const struct lsb_ar_tail *tail_in,
                     const struct lsb_cheb_epi *epi_in, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  const lsb_cheb_epi epi = epi_for(epi_in, !(flags & LSB_SP_C16) || partials || ((row_begin | s0) & 1u),
                                   "lsb_k_spmv_sell: the Chebyshev epilogue rides in the 16-bit kernel only");
  const sell_launch L = sell_prologue("lsb_k_spmv_sell", false, NULL, ns, n, grid_cap, 0, period, partials,
                                      npartials, tail_in);
  const bool nt = (flags & SP_NT) != 0;
  auto launch = [&](auto *v) { /* v: the values, of the kernel's value type */
    using VT = std::decay_t<decltype(*v)>;
    if (flags & LSB_SP_C16) {
      auto kern = nt ? k_spmv_sell16<SP_NT, VT> : k_spmv_sell16<0, VT>;
      if (epi.zout)
        kern = nt ? k_spmv_sell16<SP_NT, VT, true> : k_spmv_sell16<0, VT, true>;
      kern<<<L.g, WG, 0, s>>>(sptr, s0, ns, L.period, n, row_begin, xlen, (const short *)cols, sbase, v, vconst,
                              ulen, x, y, xdot, partials, st, L.tail, epi);
    } else {
      const auto kern = nt ? k_spmv_sell<SP_NT, VT> : k_spmv_sell<0, VT>;
      kern<<<L.g, WG, 0, s>>>(sptr, s0, ns, L.period, n, (const int *)cols, v, x, y, xdot, partials, st, L.tail);
    }
  };
  if (flags & LSB_SP_F32)
    launch((const float *)(const void *)vals);
  else
    launch(vals);
}

/* The constant-slot layout through slice templates (k_spmv_tmpl).  vals: the kept value slots
 * (fp32 when flags & LSB_SP_F32; the templates' constants are then fp32-rounded by the caller). */
void lsb_k_spmv_tmpl(unsigned flags, unsigned grid_cap, unsigned period, const struct lsb_sell16_dev *c, unsigned s0,
                     unsigned ns, unsigned n, unsigned row_begin, unsigned xlen, const double *x, double *y,
                     const double *xdot, double *partials, unsigned *npartials, const struct lsb_pcg_state *st,
                     const struct lsb_ar_tail *tail_in, const struct lsb_cheb_epi *epi_in, void *stream) {
  const lsb_cheb_epi epi = epi_for(epi_in, partials || ((row_begin | s0) & 1u),
                                   "lsb_k_spmv_tmpl: the Chebyshev epilogue takes no dot and even row offsets");
  const sell_launch L = sell_prologue("lsb_k_spmv_tmpl", false, c, ns, n, grid_cap, 0, period, partials, npartials,
                                      tail_in);
  const int f32 = (flags & LSB_SP_F32) != 0, dot_is_x = xdot && xdot == x + row_begin;
  static decltype(&k_spmv_tmpl<0, false>) const kern[3][3] = { /* [nfar][plain, Chebyshev epilogue, deferred store] */
      {k_spmv_tmpl<0, false>, k_spmv_tmpl<0, true>, k_spmv_tmpl<0, false, true>},
      {k_spmv_tmpl<1, false>, k_spmv_tmpl<1, true>, k_spmv_tmpl<1, false, true>},
      {k_spmv_tmpl<2, false>, k_spmv_tmpl<2, true>, k_spmv_tmpl<2, false, true>}};
  const int form = epi.zout ? 1 : (flags & LSB_SP_DEFER) ? 2 : 0;
  kern[c->tmpl.nfar][form]<<<L.g, WG, 0, (hipStream_t)stream>>>(
      c->sptr, s0, ns, L.period, n, row_begin, xlen, (const u4v *)c->tmpl.srec, c->tmpl.mask, c->tmpl.td, c->sbase,
      c->vals, f32, c->vconst, x, y, xdot, dot_is_x, partials, st, L.tail, epi);
}

/* The template layout walked in z-columns (k_spmv_tmpl_col): plan = xbeg[NXCD + 1], padding to 16
 * unsigneds, then nitem 16-byte items (lsb_sell_tmpl_columns).  Whole launches only (every slice of
 * the shard is in exactly one item). */
void lsb_k_spmv_tmpl_col(unsigned flags, unsigned grid_cap, unsigned period, const unsigned *plan, unsigned nitem,
                         int centre0, unsigned n, unsigned row_begin, unsigned xlen, const struct lsb_sell16_dev *c,
                         const double *x, double *y, const double *xdot, double *partials, unsigned *npartials,
                         const struct lsb_pcg_state *st, const struct lsb_ar_tail *tail_in, void *stream) {
  if (period < NXCD || !plan)
    errx(EXIT_FAILURE, "lsb_k_spmv_tmpl_col: no column plan (period %u)", period);
  const sell_launch L = sell_prologue("lsb_k_spmv_tmpl_col", true, c, nitem, n, grid_cap, 0, period, partials,
                                      npartials, tail_in);
  const int f32 = (flags & LSB_SP_F32) != 0;
  // the centre pair is the dot's operand where the dot is with the gathered vector itself (and the
  // centre base is 0: true of every operator with a diagonal; the kernel's DOT = 1 relies on it,
  // the plan builder says so in lsb_tmpl_cols.centre0)
  const int dot = !partials || !xdot ? 0 : (xdot == x + row_begin && centre0) ? 1 : 2;
  static decltype(&k_spmv_tmpl_col<1, 0>) const kern[2][3] = { /* [nfar - 1][dot] */
      {k_spmv_tmpl_col<1, 0>, k_spmv_tmpl_col<1, 1>, k_spmv_tmpl_col<1, 2>},
      {k_spmv_tmpl_col<2, 0>, k_spmv_tmpl_col<2, 1>, k_spmv_tmpl_col<2, 2>}};
  kern[c->tmpl.nfar - 1][dot]<<<L.g, WG, 0, (hipStream_t)stream>>>(
      plan, L.period, n, row_begin, xlen, c->sptr, c->tmpl.mask, c->tmpl.td, c->sbase, c->vals, f32, c->vconst, x, y,
      xdot, partials, st, L.tail);
}

void lsb_k_pcg_col_px(unsigned grid_cap, unsigned period, const unsigned *plan, unsigned nitem, unsigned n,
                      const struct lsb_sell16_dev *c, const double *r, const double *pold, double *pnew, double *x,
                      int xupd, double dc, double *partials, unsigned *npartials, struct lsb_pcg_state *st, int parity,
                      const double *parts2, unsigned nparts2, void *stream) {
  if (period < NXCD || !plan || pold == pnew)
    errx(EXIT_FAILURE, "lsb_k_pcg_col_px: no column plan (period %u) or one direction buffer", period);
  /* every workgroup resident: three per CU with two far slots per side (<= 168 VGPRs), five with one (<= 96, what
   * the kernel's launch bounds hold it to: with x it needed 102 and only four were resident, the grid's last fifth
   * ran as a second wave).  The plan's walk directions are dealt against this grid (LSB_TMPL_COL_TURN) */
  const unsigned nfar = c->tmpl.nfar;
  const sell_launch L = sell_prologue("lsb_k_pcg_col_px", true, c, nitem, n, grid_cap, LSB_TMPL_COL_GRID(nfar), period,
                                      partials, npartials, NULL);
  /* x, p' and q streamed nontemporally (NT = 3; measured against 0 / 1 / 2 on config 4: 950.5 / 950.3 / 905.7 /
   * 894.1 us per iteration, profiles/r04_px.txt -- and on config 3's cache-scale vectors, with the vectors in one
   * slab and k_pcg_col_r reversed: 100.1 / 96.5-96.8 / 97.4-97.5 against 95.6-95.9 us, profiles/r06_col_cache.txt:
   * one mask for every size, so it stays a template constant).  What "nontemporal" means for the STORES is
   * COL_ST_PX: written through the L2 (sc1 nt), not left dirty in it. */
  static decltype(&k_pcg_col_px<1, 3, false>) const kern[2][2] = { /* [nfar - 1][xupd] */
      {k_pcg_col_px<1, 3, false>, k_pcg_col_px<1, 3, true>},
      {k_pcg_col_px<2, 3, false>, k_pcg_col_px<2, 3, true>}};
  kern[nfar - 1][xupd != 0]<<<L.g, WG, 0, (hipStream_t)stream>>>(
      plan, L.period, n, c->sptr, c->tmpl.mask, c->tmpl.td, c->sbase, c->vals, c->vconst, r, pold, pnew, x, dc,
      partials, st, parity, parts2, nparts2);
}

void lsb_k_pcg_col_r(unsigned grid_cap, unsigned period, const unsigned *plan, unsigned nitem, unsigned n,
                     const struct lsb_sell16_dev *c, const double *p, double *r, double dc, struct lsb_pcg_state *st,
                     int parity, int pbuf, int xtwo, int rev, const double *pq_parts, unsigned npq, double *partials2,
                     unsigned *npartials, void *stream) {
  if (period < NXCD || !plan)
    errx(EXIT_FAILURE, "lsb_k_pcg_col_r: no column plan (period %u)", period);
  /* five workgroups per CU (launch bounds): the grid of lsb_k_pcg_col_px with one far slot per side */
  const sell_launch L = sell_prologue("lsb_k_pcg_col_r", true, c, nitem, n, grid_cap, LSB_TMPL_COL_GRID(1), period,
                                      partials2, npartials, NULL);
  const auto kern = c->tmpl.nfar == 1 ? k_pcg_col_r<1> : k_pcg_col_r<2>;
  kern<<<L.g, WG, 0, (hipStream_t)stream>>>(plan, L.period, n, c->sptr, c->tmpl.mask, c->tmpl.td, c->sbase, c->vals,
                                            c->vconst, p, r, dc, st, parity, pbuf, xtwo, rev != 0, pq_parts, npq,
                                            partials2);
}

} // extern "C"
