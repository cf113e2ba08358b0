// NSControlEnv2D on the device (reference: libs/envs/ns_control_2d.py): the 2-D periodic channel with wall blowing and suction,
// float64, one workgroup of 1024 threads per environment, the whole state in LDS for the whole launch.
//
//   k_ns2d_solve       NSControlEnv2D.solve (:359-491): wall conditions, source term (build_up_b :13-38), `nit` Jacobi sweeps
//                      (pressure_poisson_periodic :41-67), momentum update (:402-471), udiff (:472), until udiff <= u_diff_thre,
//                      max_step or the step cap; writes bulk_v = mean|u|, the step count and a status, and the state when asked
//   k_ns2d_fixed_mass  solve_fixed_mass (:493-536): two bracket solves and the bisection on F in one launch; every solve
//                      re-reads the saved state from global memory; the state is never written
//   k_ns2d_diag        the seven drag_reduction/* scalars of step (:562-581) and the top-wall pressure row
//
// Arrays are (ny, nx): row = wall-normal index, column = streamwise index, periodic in x with all nx columns distinct.
//
// LDS carve (doubles): seven planes of n = ny*nx points - u, v and p twice each (the copies un, vn, pn of the reference are
// the other plane of a pair; the roles swap instead of copying) and b - then kNs2dRed doubles for the reductions and the
// broadcast.  7 * n * 8 + 1024 <= FNO_LDS_MAX gives n <= 2907 (kNs2dMaxPoints).
//
// Points to threads: point idx = i * nx + j belongs to thread idx % 1024 (at most three points each); a thread walks its points
// in order and advances (i, j) by (1024 / nx, 1024 % nx) with one carry, so no sweep divides.
//
// Barriers per step: 1 (walls) + 1 (source term) + nit (one per sweep: the thread that computes row 1 / ny-2 also writes the
// wall row 0 / ny-1, so `p[0] = p[1]` needs no barrier of its own) + 4 (two in each of the two sums) + 1 (the decision):
// 57 at nit = 50.
//
// Arithmetic: every expression is evaluated in the reference's order with contraction off, so a value differs from numpy's
// only where a sum is taken in another order (sum(u), sum(un), mean|u|).  Those are fixed-order: thread partial over its
// points in order, xor-butterfly over the wave, the sixteen wave sums added in order by every thread.  Nothing depends on the
// batch size or on the environment's index.  The continue / stop decision is taken by thread 0 and broadcast through LDS.
#pragma once
#include <hip/hip_runtime.h>

#include "fno_dev.h"
#include "k_chanflow_step.h"

static const int kNs2dThreads = 1024;
static const int kNs2dRed = 128;                                 // doubles behind the planes: wave sums, broadcast slots
static const int kNs2dMaxPoints = (int)((FNO_LDS_MAX - kNs2dRed * sizeof(double)) / (7 * sizeof(double)));
static const int kNs2dSolveOut = 3;                              // bulk_v, steps, status
static const int kNs2dFixedOut = 6;                              // result_f, flow, error, bisections, total steps, status
static const int kNs2dDiagOut = 7;                               // the drag_reduction/* scalars in the order of `info`
enum { NS2D_CONVERGED = 0, NS2D_MAX_STEP = 1, NS2D_STEP_CAP = 2 };
enum { NS2D_FM_OK = 0, NS2D_FM_OVERFLOW = 1, NS2D_FM_STEP_CAP = 2 };

struct Ns2dGeo {
  int nx, ny, nit;
  double dx, dy, dt, rho;
};

struct Ns2dState {                 // one environment, global memory
  const double *p, *u, *v;
  const double *bc_lo, *bc_hi;     // (nx) rows or null: zero walls
};

struct Ns2dPlanes {                // LDS; planes 0 / 1 of a pair swap roles (addresses by arithmetic: an indexed pointer table
  double* base;                    // would live in scratch)
  int n;
  FNO_DEV double* u(int k) const { return base + (size_t)k * n; }
  FNO_DEV double* v(int k) const { return base + (size_t)(2 + k) * n; }
  FNO_DEV double* p(int k) const { return base + (size_t)(4 + k) * n; }
  FNO_DEV double* b() const { return base + (size_t)6 * n; }
  FNO_DEV double* red() const { return base + (size_t)7 * n; }
};

struct Ns2dResult {
  double bulk_v;
  int steps, status;
  int cu, cp;                      // which plane of the u / v pair and of the p pair holds the result
};

FNO_DEV Ns2dPlanes ns2d_carve(double* lds, int n) { return Ns2dPlanes{lds, n}; }

// sum over the workgroup (1024 threads), the same bits in every thread; red: 16 doubles
FNO_DEV double ns2d_block_sum(double v, double* red) {
  v = cf_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < kNs2dThreads / 64; ++w) s += red[w];
  return s;
}

// this thread's points in order: idx = tid, tid + 1024, ...; (i, j) advance without a division
#define NS2D_POINTS(idx, i, j) \
  for (int idx = tid, i = i0, j = j0; idx < n; idx += kNs2dThreads, i += di, j += dj, (j >= nx ? (j -= nx, ++i) : 0))

// One solve from the state `g` of one environment.  Uniform over the workgroup: every thread returns the same result.
FNO_DEV Ns2dResult ns2d_run(const Ns2dGeo& geo, const Ns2dState& g, const Ns2dPlanes& s, double F, double nu, int max_step,
                            double thre, int step_cap) {
#pragma clang fp contract(off)
  const int nx = geo.nx, ny = geo.ny, n = nx * ny, tid = threadIdx.x;
  const int di = kNs2dThreads / nx, dj = kNs2dThreads - di * nx, i0 = tid / nx, j0 = tid - i0 * nx;
  const double dx = geo.dx, dy = geo.dy, dt = geo.dt, rho = geo.rho;
  const double dx2 = dx * dx, dy2 = dy * dy, den = 2 * (dx2 + dy2), cb = dx2 * dy2 / den;
  const double tdx = 2 * dx, tdy = 2 * dy, rdt = 1 / dt;
  const double cpx = dt / (2 * rho * dx), cpy = dt / (2 * rho * dy), ddx = dt / dx2, ddy = dt / dy2, fdt = F * dt;

  __syncthreads();                                         // the planes may still be read by the previous solve's tail
  NS2D_POINTS(idx, i, j) {
    const double x = g.u[idx], y = g.v[idx];
    s.u(0)[idx] = x;
    s.v(0)[idx] = y;
    s.p(0)[idx] = g.p[idx];
    s.u(1)[idx] = x;                                       // un, vn of a launch that takes no step
    s.v(1)[idx] = y;
  }
  int cu = 0, cp = 0, steps = 0, status = NS2D_CONVERGED;
  double udiff = 1.0;
  __syncthreads();
  while (udiff > thre) {
    double *un = s.u(cu), *vn = s.v(cu), *u = s.u(cu ^ 1), *v = s.v(cu ^ 1);
    // walls (:388-397), written to both planes of the pair: the momentum update leaves the wall rows as they are
    for (int j = tid; j < nx; j += kNs2dThreads) {
      const double vl = g.bc_lo ? g.bc_lo[j] : 0.0, vh = g.bc_hi ? g.bc_hi[j] : 0.0;
      const int top = (ny - 1) * nx + j;
      un[j] = 0.0; un[top] = 0.0; vn[j] = vl; vn[top] = vh;
      u[j] = 0.0; u[top] = 0.0; v[j] = vl; v[top] = vh;
    }
    __syncthreads();
    // source term (:13-38)
    NS2D_POINTS(at, i, j) {
      if (i < 1 || i > ny - 2) continue;
      const int l = at + (j == 0 ? nx - 1 : -1), r = at + (j == nx - 1 ? 1 - nx : 1);
      const double dudx = (un[r] - un[l]) / tdx, dvdy = (vn[at + nx] - vn[at - nx]) / tdy;
      const double cross = (un[at + nx] - un[at - nx]) / tdy * (vn[r] - vn[l]) / tdx;
      s.b()[at] = rho * (rdt * (dudx + dvdy) - dudx * dudx - 2 * cross - dvdy * dvdy);
    }
    __syncthreads();
    // pressure (:41-67): every sweep reads the previous sweep's plane everywhere
    for (int q = 0; q < geo.nit; ++q) {
      const double* pn = s.p(cp);
      double* p = s.p(cp ^ 1);
      NS2D_POINTS(at, i, j) {
        if (i < 1 || i > ny - 2) continue;
        const int l = at + (j == 0 ? nx - 1 : -1), r = at + (j == nx - 1 ? 1 - nx : 1);
        const double val = ((pn[r] + pn[l]) * dy2 + (pn[at + nx] + pn[at - nx]) * dx2) / den - cb * s.b()[at];
        p[at] = val;
        if (i == 1) p[at - nx] = val;                      // p[0, :] = p[1, :]
        if (i == ny - 2) p[at + nx] = val;                 // p[-1, :] = p[-2, :]
      }
      cp ^= 1;
      __syncthreads();
    }
    // momentum (:402-471)
    const double* p = s.p(cp);
    double su = 0.0, sun = 0.0;
    NS2D_POINTS(at, i, j) {
      if (i >= 1 && i <= ny - 2) {
        const int l = at + (j == 0 ? nx - 1 : -1), r = at + (j == nx - 1 ? 1 - nx : 1);
        const double uc = un[at], vc = vn[at], ul = un[l], ur = un[r], ud = un[at - nx], uu = un[at + nx];
        const double vl = vn[l], vr = vn[r], vd = vn[at - nx], vu = vn[at + nx];
        u[at] = uc - uc * dt / dx * (uc - ul) - vc * dt / dy * (uc - ud) - cpx * (p[r] - p[l]) +
                nu * (ddx * (ur - 2 * uc + ul) + ddy * (uu - 2 * uc + ud)) + fdt;
        v[at] = vc - uc * dt / dx * (vc - vl) - vc * dt / dy * (vc - vd) - cpy * (p[at + nx] - p[at - nx]) +
                nu * (ddx * (vr - 2 * vc + vl) + ddy * (vu - 2 * vc + vd));
      }
      su += u[at];                                         // a thread reads back what it wrote itself, or a wall value
      sun += un[at];
    }
    su = ns2d_block_sum(su, s.red());
    sun = ns2d_block_sum(sun, s.red() + 16);
    cu ^= 1;
    ++steps;
    if (tid == 0) {                                        // (:472-477) one decision per workgroup
      const double ud = (su - sun) / su;
      int go = 1, st = NS2D_CONVERGED;
      if (steps > step_cap) { go = 0; st = NS2D_STEP_CAP; }
      else if (max_step > 1 && steps >= max_step) { go = 0; st = NS2D_MAX_STEP; }
      else if (!(ud > thre)) go = 0;
      s.red()[32] = ud;
      s.red()[33] = (double)go;
      s.red()[34] = (double)st;
    }
    __syncthreads();
    udiff = s.red()[32];
    status = __builtin_amdgcn_readfirstlane((int)s.red()[34]);
    if (__builtin_amdgcn_readfirstlane((int)s.red()[33]) == 0) break;
  }
  double sa = 0.0;
  NS2D_POINTS(at, i, j) sa += fabs(s.u(cu)[at]);
  Ns2dResult res;
  res.bulk_v = ns2d_block_sum(sa, s.red() + 48) / (double)n;
  res.steps = steps;
  res.status = status;
  res.cu = cu;
  res.cp = cp;
  return res;
}

struct Ns2dSolveArgs {
  double *p, *u, *v;               // (B, ny, nx) in / out (written when `update` and the cap was not hit)
  double *un, *vn;                 // (B, ny, nx) out or null
  const double *F, *nu;            // (B)
  const double *bc_lo, *bc_hi;     // (B, nx) or null
  double* out;                     // (B, kNs2dSolveOut)
  int max_step, step_cap, update;
  double thre;
};

__global__ __launch_bounds__(kNs2dThreads) void k_ns2d_solve(Ns2dGeo geo, Ns2dSolveArgs a) {
  extern __shared__ double ns2d_lds[];
  const int b = blockIdx.x, n = geo.nx * geo.ny, tid = threadIdx.x;
  const Ns2dPlanes s = ns2d_carve(ns2d_lds, n);
  const size_t at = (size_t)b * n, row = (size_t)b * geo.nx;
  const Ns2dState g = {a.p + at, a.u + at, a.v + at, a.bc_lo ? a.bc_lo + row : nullptr, a.bc_hi ? a.bc_hi + row : nullptr};
  const Ns2dResult res = ns2d_run(geo, g, s, a.F[b], a.nu[b], a.max_step, a.thre, a.step_cap);
  if (a.update && res.status != NS2D_STEP_CAP)            // the reference raises before it stores anything
    for (int idx = tid; idx < n; idx += kNs2dThreads) {
      a.u[at + idx] = s.u(res.cu)[idx];
      a.v[at + idx] = s.v(res.cu)[idx];
      a.p[at + idx] = s.p(res.cp)[idx];
      if (a.un) a.un[at + idx] = s.u(res.cu ^ 1)[idx];
      if (a.vn) a.vn[at + idx] = s.v(res.cu ^ 1)[idx];
    }
  if (tid == 0) {
    double* o = a.out + (size_t)b * kNs2dSolveOut;
    o[0] = res.bulk_v; o[1] = (double)res.steps; o[2] = (double)res.status;
  }
}

struct Ns2dFixedArgs {
  const double *p, *u, *v;         // (B, ny, nx), read only
  const double *F, *nu;            // (B): F is what an overflow returns
  const double *target, *min_f, *max_f;      // (B)
  const double *bc_lo, *bc_hi;
  double* out;                     // (B, kNs2dFixedOut)
  int step_cap, max_bisect;
  double thre, err_thre;
};

__global__ __launch_bounds__(kNs2dThreads) void k_ns2d_fixed_mass(Ns2dGeo geo, Ns2dFixedArgs a) {
  extern __shared__ double ns2d_lds[];
  const int b = blockIdx.x, n = geo.nx * geo.ny;
  const Ns2dPlanes s = ns2d_carve(ns2d_lds, n);
  const size_t at = (size_t)b * n, row = (size_t)b * geo.nx;
  const Ns2dState g = {a.p + at, a.u + at, a.v + at, a.bc_lo ? a.bc_lo + row : nullptr, a.bc_hi ? a.bc_hi + row : nullptr};
  const double nu = a.nu[b], target = a.target[b];
  double lo = a.min_f[b], hi = a.max_f[b];
  double result = a.F[b], flow = target, err = 0.0;
  int nb = 0, status = NS2D_FM_OK;
  long long total = 0;
  // every quantity below is the same in all threads (ns2d_run broadcasts), so the control flow is uniform.  Solve 0 and 1 are
  // the bracket at min_f and max_f, every later one a bisection (one call site: the solver is inlined once)
  double min_flow = 0.0, f = lo;
  for (int k = 0;; ++k) {
    const Ns2dResult r = ns2d_run(geo, g, s, f, nu, -1, a.thre, a.step_cap);
    total += r.steps;
    if (r.status == NS2D_STEP_CAP) { status = NS2D_FM_STEP_CAP; break; }
    if (k == 0) { min_flow = r.bulk_v; f = hi; continue; }
    if (k == 1) {
      if (target < min_flow || target > r.bulk_v) { status = NS2D_FM_OVERFLOW; break; }      // (:509-512) returns (self.F, target, 0)
      flow = 0.0;                                          // error = inf until the first bisection (:516): nb == 0 below
    } else {                                              // (:525-533)
      flow = r.bulk_v;
      err = fabs(flow - target);
      if (flow < target) lo = f; else hi = f;
      result = f;
      ++nb;
    }
    if (!(nb < a.max_bisect && (nb == 0 || err > a.err_thre))) break;      // (:519)
    f = (lo + hi) / 2;
  }
  if (threadIdx.x == 0) {
    double* o = a.out + (size_t)b * kNs2dFixedOut;
    o[0] = result; o[1] = flow; o[2] = err; o[3] = (double)nb; o[4] = (double)total; o[5] = (double)status;
  }
}

// the seven scalars of `info` (:562-581) and pressure_top = p[-1, :]; cal_div reads the fixed indices 10 and 9 (:169-172), so
// the host refuses grids below 11 x 11.  dpdx (B) or null: drag_reduction/3_2_dPdx_required is -1 without fix_flow.
__global__ __launch_bounds__(256) void k_ns2d_diag(Ns2dGeo geo, const double* p, const double* u, const double* v, const double* nu,
                                                   const double* dpdx, double* out, double* ptop) {
#pragma clang fp contract(off)
  __shared__ double red[4];
  const int nx = geo.nx, ny = geo.ny, n = nx * ny, b = blockIdx.x, tid = threadIdx.x;
  const double *pb = p + (size_t)b * n, *ub = u + (size_t)b * n, *vb = v + (size_t)b * n;
  double au = 0.0, av = 0.0, uu = 0.0, vv = 0.0, sh = 0.0, pt = 0.0;
  for (int idx = tid; idx < n; idx += 256) {
    const double x = ub[idx], y = vb[idx];
    au += fabs(x); av += fabs(y); uu += x * x; vv += y * y;
  }
  const double visc = nu[b];
  for (int j = tid; j < nx; j += 256) {
    const int top = (ny - 1) * nx + j;
    const double dudy = (ub[top - nx] - ub[top - 2 * nx]) / geo.dy;      // cal_dudy's last entry (:205-217)
    sh += -ub[top] * vb[top] + visc * dudy;
    pt += pb[top];
    ptop[(size_t)b * nx + j] = pb[top];
  }
  au = cf_block_sum(au, red); av = cf_block_sum(av, red); uu = cf_block_sum(uu, red); vv = cf_block_sum(vv, red);
  sh = cf_block_sum(sh, red); pt = cf_block_sum(pt, red);
  if (tid == 0) {
    double* o = out + (size_t)b * kNs2dDiagOut;
    const double div = (ub[10 * nx + 10] - ub[9 * nx + 10]) / geo.dx + (vb[10 * nx + 10] - vb[10 * nx + 9]) / geo.dy;
    double reward = -fabs(div);                            // reward_div (:225-229)
    if (reward < -100.0) reward = -100.0;
    o[0] = fabs(sh / (double)nx);
    o[1] = au / (double)n;
    o[2] = av / (double)n;
    o[3] = pt / (double)nx;
    o[4] = dpdx ? dpdx[b] : -1.0;
    o[5] = reward;
    o[6] = sqrt(vv) + sqrt(uu);
  }
}
