// Geometric multigrid V-cycle on a constant-coefficient grid (LSB_PRECOND_GMG): z = M^-1 r as one symmetric V-cycle
// from a zero initial guess with damped Jacobi smoothing.  The rules -- levels, the far-face correction of the
// diagonal, P, R = sigma P^T, the weights -- are lsb_gmg.c's; hip_gmg_drv.c enqueues the launches below.  On level l,
// with nu = opts.amg_sweeps and w_i = omega / D_i:
//     x = w b;  (nu - 1) x  x += w (b - A x)
//     r = b - A x;  b_c = sigma P^T r;  recurse (the coarsest level: x_c = coarse_inv b_c, lsb_k_amg_dense)
//     x += P x_c;  nu x  x += w (b - A x)
//
// There is NO matrix array on any level: the stencil, c, the points per dimension, the pitch and the 2^dim diagonals
// and weights arrive as kernel arguments (struct lsb_gmg_lv, by value), so every kernel streams vectors only.  One
// lane per point along x; no atomics, every output is one lane's fixed-order sum, so z is bitwise repeatable.
//
// Plain steps, one launch each (any nu):
//   k_gmg_first     x = w b
//   k_gmg_sweep     y = x + w (b - A x), out of place (the driver ping-pongs two buffers)
//   k_gmg_restrict  b_c = sigma P^T (b - A x): a coarse point forms the 3^dim fine residuals it needs
//   k_gmg_prolong   x += P x_c in place (point i reads only x_i of x)
// Fused steps for nu = 1, the hot path:
//   k_gmg_down      x = w b is pointwise in b, so r = b - A (w b) and its restriction need only b: a lane per coarse
//                   point reads b (the 5^dim window around its fine point, through the caches), writes b_c and the x of
//                   the fine points it owns.  Per fine row: b read, x written, b_c / 2^dim written.
//   k_gmg_up        u = x + P x_c on a tile with a one-point halo in LDS, then the one sweep on it: per fine row x, b
//                   and x_c / 2^dim read, the result written.
// What a point's w, D, A x, P and P^T are is ONE device function each (gmg_mask, gmg_ax, gmg_nbsum, gmg_resid,
// gmg_restrict_at, gmg_prolong_at, gmg_sweep_at), used by the plain and by the fused kernel, and the file is compiled
// with floating-point contraction off -- every fma below is written out -- so the two paths give the SAME bits
// (LSBENCH_HIP_GMG_FUSE=0 selects the plain steps; tests compare).
//
// Launch bounds and sizes: the flat kernels run GMG_WG = 256 threads, a lane per point (or coarse point) along x, no
// LDS.  k_gmg_up runs GMG_UP = 512 threads on a tile of 64 x 8 (2-D) or 32 x 4 x 4 (3-D) points: with the halo 66 x 10
// = 660 or 34 x 6 x 6 = 1224 doubles of LDS, 5.2 / 9.6 KiB per workgroup, far below what would bound the 4 workgroups
// of 8 waves a CU can hold (160 KiB); lanes walk x, consecutive doubles, so the tile's reads and writes are free of
// bank conflicts.  The halo costs 1.29 x (2-D) / 2.06 x (3-D, faces only: edges and corners are not formed) the
// tile's own evaluations of x + P x_c, all served by L2.  No kernel spills (tests/test_gmg_resources.py).
// Every kernel is a no-op once the solve's state has left RUNNING.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hip_kcommon.h"

#pragma clang fp contract(off)

#define GMG_WG 256
#define GMG_UP 512

// ---- a point's numbers ------------------------------------------------------------------------------------------
template <int DIM> __device__ __forceinline__ size_t gmg_idx(const lsb_gmg_lv &lv, unsigned i, unsigned j, unsigned k) {
  return DIM == 3 ? ((size_t)k * lv.n[1] + j) * lv.pitch + i : (size_t)j * lv.pitch + i;
}

// the far faces the point lies on: selects its diagonal D and its weight w
template <int DIM> __device__ __forceinline__ unsigned gmg_mask(const lsb_gmg_lv &lv, unsigned i, unsigned j, unsigned k) {
  unsigned m = (i == lv.n[0] - 1 ? 1u : 0u) | (j == lv.n[1] - 1 ? 2u : 0u);
  if (DIM == 3)
    m |= k == lv.n[2] - 1 ? 4u : 0u;
  return m;
}

// the level's vectors as the stencil reads them: a stored x, or x = w b formed on the fly (the way down)
struct gmg_stored {
  const double *x;
  template <int DIM> __device__ __forceinline__ double at(const lsb_gmg_lv &lv, unsigned i, unsigned j, unsigned k) const {
    return x[gmg_idx<DIM>(lv, i, j, k)];
  }
};
__device__ __forceinline__ double gmg_first_at(double w, double b) { return w * b; }
struct gmg_wb {
  const double *b;
  template <int DIM> __device__ __forceinline__ double at(const lsb_gmg_lv &lv, unsigned i, unsigned j, unsigned k) const {
    return gmg_first_at(lv.w[gmg_mask<DIM>(lv, i, j, k)], b[gmg_idx<DIM>(lv, i, j, k)]);
  }
};

// the neighbours' sum in its one order: (x- + x+) + (y- + y+) [+ (z- + z+)], 0 for a neighbour outside
__device__ __forceinline__ double gmg_nbsum2(double xm, double xp, double ym, double yp) { return (xm + xp) + (ym + yp); }
__device__ __forceinline__ double gmg_nbsum3(double s2, double zm, double zp) { return s2 + (zm + zp); }
template <int DIM, typename X>
__device__ __forceinline__ double gmg_nbsum(const lsb_gmg_lv &lv, const X &x, unsigned i, unsigned j, unsigned k) {
  const double xm = i > 0 ? x.template at<DIM>(lv, i - 1, j, k) : 0.0;
  const double xp = i + 1 < lv.n[0] ? x.template at<DIM>(lv, i + 1, j, k) : 0.0;
  const double ym = j > 0 ? x.template at<DIM>(lv, i, j - 1, k) : 0.0;
  const double yp = j + 1 < lv.n[1] ? x.template at<DIM>(lv, i, j + 1, k) : 0.0;
  double s = gmg_nbsum2(xm, xp, ym, yp);
  if (DIM == 3) {
    const double zm = k > 0 ? x.template at<DIM>(lv, i, j, k - 1) : 0.0;
    const double zp = k + 1 < lv.n[2] ? x.template at<DIM>(lv, i, j, k + 1) : 0.0;
    s = gmg_nbsum3(s, zm, zp);
  }
  return s;
}

// (A x)_i from x_i and its neighbours' sum; the sweep's result
__device__ __forceinline__ double gmg_ax(double D, double c, double xc, double nb) { return fma(D, xc, -(c * nb)); }
__device__ __forceinline__ double gmg_sweep_at(double D, double w, double c, double xc, double nb, double b) {
  return fma(w, b - gmg_ax(D, c, xc, nb), xc);
}

// r_i = b_i - (A x)_i
template <int DIM, typename X>
__device__ __forceinline__ double gmg_resid(const lsb_gmg_lv &lv, const X &x, const double *b, unsigned i, unsigned j,
                                            unsigned k) {
  const unsigned m = gmg_mask<DIM>(lv, i, j, k);
  return b[gmg_idx<DIM>(lv, i, j, k)] - gmg_ax(lv.D[m], lv.c, x.template at<DIM>(lv, i, j, k), gmg_nbsum<DIM>(lv, x, i, j, k));
}

// the weight of fine point 2 J + 1 + a (a = -1, 0, 1) of dimension d in coarse point J, 0 where there is no such point
__device__ __forceinline__ double gmg_rweight(const lsb_gmg_lv &lv, int d, unsigned J, int a) {
  if (a <= 0)
    return a == 0 ? 1.0 : 0.5;
  const unsigned f = 2 * J + 2;
  return f + 1 < lv.n[d] ? 0.5 : (f + 1 == lv.n[d] ? lv.wlast[d] : 0.0);
}

// (sigma P^T r)_J, r formed point by point; the terms in the order z, y, x
template <int DIM, typename X>
__device__ __forceinline__ double gmg_restrict_at(const lsb_gmg_lv &lv, const X &x, const double *b, unsigned I, unsigned J,
                                                  unsigned K) {
  double s = 0.0;
  constexpr int UY = DIM == 3 ? 1 : 3; // 3-D: a line of 3 residuals at a time (all 27 unrolled spill in k_gmg_down)
#pragma unroll 1
  for (int az = (DIM == 3 ? -1 : 0); az <= (DIM == 3 ? 1 : 0); az++) {
    const double wz = DIM == 3 ? gmg_rweight(lv, 2, K, az) : 1.0;
    if (wz == 0.0)
      continue;
#pragma unroll UY
    for (int ay = -1; ay <= 1; ay++) {
      const double wy = gmg_rweight(lv, 1, J, ay);
      if (wy == 0.0)
        continue;
#pragma unroll
      for (int ax = -1; ax <= 1; ax++) {
        const double wx = gmg_rweight(lv, 0, I, ax);
        if (wx == 0.0)
          continue;
        const double r = gmg_resid<DIM>(lv, x, b, 2 * I + 1 + ax, 2 * J + 1 + ay, DIM == 3 ? 2 * K + 1 + az : 0u);
        s = fma((wz * wy) * wx, r, s);
      }
    }
  }
  return lv.sigma * s;
}

// the (at most two) coarse points fine point i of dimension d takes from, with their weights (0: none)
__device__ __forceinline__ void gmg_pweights(const lsb_gmg_lv &lv, int d, unsigned i, unsigned (&j)[2], double (&w)[2]) {
  if (i & 1u) {
    j[0] = i / 2, w[0] = 1.0, j[1] = 0, w[1] = 0.0;
  } else if (i + 1 == lv.n[d]) { // the last point of an odd n
    j[0] = lv.nc[d] - 1, w[0] = lv.wlast[d], j[1] = 0, w[1] = 0.0;
  } else {
    j[0] = i ? i / 2 - 1 : 0, w[0] = i ? 0.5 : 0.0, j[1] = i / 2, w[1] = 0.5;
  }
}

// (P x_c)_i; the terms in the order z, y, x.  x_c has the next level's pitch, its nc[0]
template <int DIM>
__device__ __forceinline__ double gmg_prolong_at(const lsb_gmg_lv &lv, const double *xc, unsigned i, unsigned j, unsigned k) {
  unsigned jx[2], jy[2], jz[2] = {0, 0};
  double wx[2], wy[2], wz[2] = {1.0, 0.0};
  gmg_pweights(lv, 0, i, jx, wx);
  gmg_pweights(lv, 1, j, jy, wy);
  if (DIM == 3)
    gmg_pweights(lv, 2, k, jz, wz);
  double s = 0.0;
#pragma unroll
  for (int c = 0; c < (DIM == 3 ? 2 : 1); c++) {
    if (wz[c] == 0.0)
      continue;
#pragma unroll
    for (int b = 0; b < 2; b++) {
      if (wy[b] == 0.0)
        continue;
#pragma unroll
      for (int a = 0; a < 2; a++) {
        if (wx[a] == 0.0)
          continue;
        const size_t at = ((size_t)jz[c] * lv.nc[1] + jy[b]) * lv.nc[0] + jx[a];
        s = fma((wz[c] * wy[b]) * wx[a], xc[at], s);
      }
    }
  }
  return s;
}
__device__ __forceinline__ double gmg_add_at(double x, double px) { return x + px; }

// flat thread id -> point: lanes along x over the pitch, then the lines.  false: beyond the grid.  In 32 bits: a level
// has fewer than 2^31 elements (the solver's int32 row indices), so the grid's last thread id is below 2^31 + GMG_WG
template <int DIM>
__device__ __forceinline__ bool gmg_point(unsigned nx, unsigned ny, unsigned nz, unsigned &i, unsigned &j, unsigned &k) {
  const unsigned t = blockIdx.x * GMG_WG + threadIdx.x;
  const unsigned line = t / nx;
  i = t - line * nx;
  if (DIM == 3)
    k = line / ny, j = line - k * ny;
  else
    k = 0, j = line;
  return DIM == 3 ? k < nz : j < ny;
}

// ---- the plain steps --------------------------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(GMG_WG) void k_gmg_first(const lsb_gmg_lv lv, const double *__restrict__ b,
                                                      double *__restrict__ x, const struct lsb_pcg_state *st) {
  if (st && st->status)
    return;
  unsigned i, j, k;
  if (!gmg_point<DIM>(lv.pitch, lv.n[1], lv.n[2], i, j, k))
    return;
  const size_t at = gmg_idx<DIM>(lv, i, j, k);
  x[at] = i < lv.n[0] ? gmg_first_at(lv.w[gmg_mask<DIM>(lv, i, j, k)], b[at]) : 0.0;
}

template <int DIM>
__global__ __launch_bounds__(GMG_WG) void k_gmg_sweep(const lsb_gmg_lv lv, const double *__restrict__ xin,
                                                      const double *__restrict__ b, double *__restrict__ y,
                                                      const struct lsb_pcg_state *st) {
  if (st && st->status)
    return;
  unsigned i, j, k;
  if (!gmg_point<DIM>(lv.pitch, lv.n[1], lv.n[2], i, j, k))
    return;
  const size_t at = gmg_idx<DIM>(lv, i, j, k);
  if (i >= lv.n[0]) {
    y[at] = 0.0;
    return;
  }
  const unsigned m = gmg_mask<DIM>(lv, i, j, k);
  const gmg_stored x = {xin};
  y[at] = gmg_sweep_at(lv.D[m], lv.w[m], lv.c, xin[at], gmg_nbsum<DIM>(lv, x, i, j, k), b[at]);
}

template <int DIM>
__global__ __launch_bounds__(GMG_WG) void k_gmg_restrict(const lsb_gmg_lv lv, const double *__restrict__ xin,
                                                         const double *__restrict__ b, double *__restrict__ bc,
                                                         const struct lsb_pcg_state *st) {
  if (st && st->status)
    return;
  unsigned I, J, K;
  if (!gmg_point<DIM>(lv.nc[0], lv.nc[1], lv.nc[2], I, J, K))
    return;
  const gmg_stored x = {xin};
  bc[((size_t)K * lv.nc[1] + J) * lv.nc[0] + I] = gmg_restrict_at<DIM>(lv, x, b, I, J, K);
}

template <int DIM>
__global__ __launch_bounds__(GMG_WG) void k_gmg_prolong(const lsb_gmg_lv lv, double *__restrict__ x,
                                                        const double *__restrict__ xc, const struct lsb_pcg_state *st) {
  if (st && st->status)
    return;
  unsigned i, j, k;
  if (!gmg_point<DIM>(lv.pitch, lv.n[1], lv.n[2], i, j, k) || i >= lv.n[0])
    return;
  const size_t at = gmg_idx<DIM>(lv, i, j, k);
  x[at] = gmg_add_at(x[at], gmg_prolong_at<DIM>(lv, xc, i, j, k));
}

// ---- the fused steps --------------------------------------------------------------------------------------------
// the way down at nu = 1.  A lane per coarse point; it owns the fine points 2 J, 2 J + 1 of every dimension, the last
// coarse point of an odd n also 2 J + 2: every fine point has exactly one owner
template <int DIM>
__global__ __launch_bounds__(GMG_WG) void k_gmg_down(const lsb_gmg_lv lv, const double *__restrict__ b,
                                                     double *__restrict__ x, double *__restrict__ bc,
                                                     const struct lsb_pcg_state *st) {
  if (st && st->status)
    return;
  unsigned I, J, K;
  if (!gmg_point<DIM>(lv.nc[0], lv.nc[1], lv.nc[2], I, J, K))
    return;
  const gmg_wb xb = {b};
  bc[((size_t)K * lv.nc[1] + J) * lv.nc[0] + I] = gmg_restrict_at<DIM>(lv, xb, b, I, J, K);
  const unsigned ex = I + 1 == lv.nc[0] ? lv.n[0] : 2 * I + 2, ey = J + 1 == lv.nc[1] ? lv.n[1] : 2 * J + 2;
  const unsigned k0 = DIM == 3 ? 2 * K : 0u, ez = DIM == 3 ? (K + 1 == lv.nc[2] ? lv.n[2] : 2 * K + 2) : 1u;
  for (unsigned k = k0; k < ez; k++)
    for (unsigned j = 2 * J; j < ey; j++)
      for (unsigned i = 2 * I; i < ex; i++)
        x[gmg_idx<DIM>(lv, i, j, k)] = xb.template at<DIM>(lv, i, j, k);
}

// the way up at nu = 1: u = x + P x_c on the tile and its face halo in LDS (0 outside the grid), then the sweep
template <int DIM> struct gmg_tile {
  static constexpr int TX = DIM == 3 ? 32 : 64, TY = DIM == 3 ? 4 : 8, TZ = DIM == 3 ? 4 : 1;
  static constexpr int HX = TX + 2, HY = TY + 2, HZ = DIM == 3 ? TZ + 2 : 1;
};

template <int DIM>
__global__ __launch_bounds__(GMG_UP) void k_gmg_up(const lsb_gmg_lv lv, const double *__restrict__ xin,
                                                   const double *__restrict__ b, const double *__restrict__ xc,
                                                   double *__restrict__ y, unsigned tiles_x, unsigned tiles_y,
                                                   const struct lsb_pcg_state *st) {
  typedef gmg_tile<DIM> T;
  static_assert(T::TX * T::TY * T::TZ == GMG_UP, "a lane per point of the tile");
  __shared__ double u[T::HZ][T::HY][T::HX];
  if (st && st->status)
    return;
  const unsigned bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x % tiles_y, bz = blockIdx.x / tiles_x / tiles_y;
  const int x0 = (int)(bx * T::TX), y0 = (int)(by * T::TY), z0 = (int)(bz * T::TZ);
  const int nz = DIM == 3 ? (int)lv.n[2] : 1;
  for (int h = (int)threadIdx.x; h < T::HX * T::HY * T::HZ; h += GMG_UP) {
    const int hx = h % T::HX, hy = h / T::HX % T::HY, hz = h / (T::HX * T::HY);
    const int faces = (hx == 0 || hx == T::HX - 1) + (hy == 0 || hy == T::HY - 1) + (DIM == 3 && (hz == 0 || hz == T::HZ - 1));
    if (faces > 1) // edges and corners of the halo: no point of the tile reads them
      continue;
    const int gi = x0 + hx - 1, gj = y0 + hy - 1, gk = DIM == 3 ? z0 + hz - 1 : 0;
    double v = 0.0;
    if (gi >= 0 && gi < (int)lv.n[0] && gj >= 0 && gj < (int)lv.n[1] && gk >= 0 && gk < nz)
      v = gmg_add_at(xin[gmg_idx<DIM>(lv, gi, gj, gk)], gmg_prolong_at<DIM>(lv, xc, gi, gj, gk));
    u[hz][hy][hx] = v;
  }
  __syncthreads();
  const int tx = (int)threadIdx.x % T::TX, ty = (int)threadIdx.x / T::TX % T::TY, tz = (int)threadIdx.x / (T::TX * T::TY);
  const unsigned i = (unsigned)(x0 + tx), j = (unsigned)(y0 + ty), k = (unsigned)(z0 + tz);
  if (i >= lv.pitch || j >= lv.n[1] || (int)k >= nz)
    return;
  const size_t at = gmg_idx<DIM>(lv, i, j, k);
  if (i >= lv.n[0]) {
    y[at] = 0.0;
    return;
  }
  const int cz = DIM == 3 ? tz + 1 : 0;
  double nb = gmg_nbsum2(u[cz][ty + 1][tx], u[cz][ty + 1][tx + 2], u[cz][ty][tx + 1], u[cz][ty + 2][tx + 1]);
  if (DIM == 3)
    nb = gmg_nbsum3(nb, u[tz][ty + 1][tx + 1], u[tz + 2][ty + 1][tx + 1]);
  const unsigned m = gmg_mask<DIM>(lv, i, j, k);
  y[at] = gmg_sweep_at(lv.D[m], lv.w[m], lv.c, u[cz][ty + 1][tx + 1], nb, b[at]);
}

template <int DIM>
static void gmg_launch_up(const struct lsb_gmg_lv *lv, const double *x, const double *b, const double *xc, double *y,
                          const struct lsb_pcg_state *st, hipStream_t stream) {
  typedef gmg_tile<DIM> T;
  const unsigned tx = div_up(lv->pitch, T::TX), ty = div_up(lv->n[1], T::TY), tz = div_up(lv->n[2], T::TZ);
  k_gmg_up<DIM><<<tx * ty * tz, GMG_UP, 0, stream>>>(*lv, x, b, xc, y, tx, ty, st);
}

extern "C" {

static unsigned gmg_grid(const struct lsb_gmg_lv *lv, int coarse) {
  const unsigned long long pts = coarse ? (unsigned long long)lv->nc[0] * lv->nc[1] * lv->nc[2]
                                        : (unsigned long long)lv->pitch * lv->n[1] * lv->n[2];
  return (unsigned)((pts + GMG_WG - 1) / GMG_WG);
}

#define GMG_DIM(dim, CALL)                                              \
  do {                                                                  \
    if ((dim) == 2) {                                                   \
      constexpr int DIM = 2;                                            \
      CALL;                                                             \
    } else if ((dim) == 3) {                                            \
      constexpr int DIM = 3;                                            \
      CALL;                                                             \
    } else                                                              \
      errx(EXIT_FAILURE, "hip_gmg: no kernels for dimension %u", dim);  \
  } while (0)

void lsb_k_gmg_first(unsigned dim, const struct lsb_gmg_lv *lv, const double *b, double *x,
                     const struct lsb_pcg_state *st, void *stream) {
  GMG_DIM(dim, (k_gmg_first<DIM><<<gmg_grid(lv, 0), GMG_WG, 0, (hipStream_t)stream>>>(*lv, b, x, st)));
}

void lsb_k_gmg_sweep(unsigned dim, const struct lsb_gmg_lv *lv, const double *xin, const double *b, double *y,
                     const struct lsb_pcg_state *st, void *stream) {
  GMG_DIM(dim, (k_gmg_sweep<DIM><<<gmg_grid(lv, 0), GMG_WG, 0, (hipStream_t)stream>>>(*lv, xin, b, y, st)));
}

void lsb_k_gmg_restrict(unsigned dim, const struct lsb_gmg_lv *lv, const double *x, const double *b, double *bc,
                        const struct lsb_pcg_state *st, void *stream) {
  GMG_DIM(dim, (k_gmg_restrict<DIM><<<gmg_grid(lv, 1), GMG_WG, 0, (hipStream_t)stream>>>(*lv, x, b, bc, st)));
}

void lsb_k_gmg_prolong(unsigned dim, const struct lsb_gmg_lv *lv, double *x, const double *xc,
                       const struct lsb_pcg_state *st, void *stream) {
  GMG_DIM(dim, (k_gmg_prolong<DIM><<<gmg_grid(lv, 0), GMG_WG, 0, (hipStream_t)stream>>>(*lv, x, xc, st)));
}

void lsb_k_gmg_down(unsigned dim, const struct lsb_gmg_lv *lv, const double *b, double *x, double *bc,
                    const struct lsb_pcg_state *st, void *stream) {
  GMG_DIM(dim, (k_gmg_down<DIM><<<gmg_grid(lv, 1), GMG_WG, 0, (hipStream_t)stream>>>(*lv, b, x, bc, st)));
}

void lsb_k_gmg_up(unsigned dim, const struct lsb_gmg_lv *lv, const double *x, const double *b, const double *xc,
                  double *y, const struct lsb_pcg_state *st, void *stream) {
  GMG_DIM(dim, (gmg_launch_up<DIM>(lv, x, b, xc, y, st, (hipStream_t)stream)));
}

} // extern "C"
