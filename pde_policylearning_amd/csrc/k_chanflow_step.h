// Channel-flow environment step in fp64: boundary-controlled RK3 advance, fractional-step projection, wall-pressure
// observation and the drag / divergence diagnostics (reference: NSControlEnvMatlab.time_advance_RK3_py
// libs/envs/control_env.py:533-580, compute_projection_step :582-613, compute_pressure_py :196-229, the scores :186-303).
//
// The reference solves, per projection, Nx*Nz dense complex (Ny-1)x(Ny-1) systems.  The matrices are DD + (kxx+kzz) I: real,
// tridiagonal and fixed per grid, so the host factors them once (fno_chanflow_poisson_pack) and a solve is a forward and a
// back recurrence per wavenumber pair.  The fields are real, so only kz <= Nz/2 is kept (the other half is its conjugate
// and the systems are even in kx, kz).
//
// Chain of one projection (h = complex (B, Ny-1, Nx*Nzh), Nzh = Nz/2+1):
//   k_chanflow_stage    workgroup = (y-plane j, sample): [stage state X0 + ca F1 + cb Fs, wall condition, write] ->
//                       divergence rows -> DFT along z -> DFT along x (both in LDS) -> h[b, j]
//   k_chanflow_solve    workgroup = 32 wavenumber columns x all Ny-1 rows AND their factors staged in LDS by all threads; one
//                       wave runs the 64 real recurrences (re, im of 32 columns) on conflict-free rows of 64 doubles, no
//                       global access inside the chain; h -> p_hat in place
//   k_chanflow_correct  workgroup = (y-plane j, sample): inverse transforms of p_hat[j] and p_hat[j] - p_hat[j-1], the three
//                       gradient corrections, the wall condition; on the last RK stage also the xz-sum of the new U row
//   k_chanflow_pressure the same inverse on -(p_hat[a] + p_hat[b])/2 for the two wall observations (and every plane of P
//                       when the full field is asked for)
//   k_chanflow_bulk     bulk-velocity correction and the dPdx update from the per-row sums, all on the device
//   k_chanflow_diag     one workgroup per sample: every scalar of the environment's `info`
// The transforms are table-driven direct DFTs (twiddles from the packed table): N <= 128 and the plane is a few KB, so a
// workgroup's transform is a few hundred FMAs per thread; every launch at B = 1 is latency-bound, not FLOP-bound.
#pragma once
#include <hip/hip_runtime.h>

#include "fno_dev.h"
#include "k_chanflow.h"

static const int kCfTile = 32;        // wavenumber columns per solve workgroup (64 real recurrences = one wave)
static const int kCfDiag = 12;        // doubles per sample written by k_chanflow_diag (include/fnoengine.h)

// offsets (in doubles) into the packed Poisson table; every section starts on a 16-byte boundary
struct ChanflowTab {
  const double* base;
  int twx, twz, wgt, trap, sub, fac;      // twiddles e^{-2 pi i m / N} (x, z), c2r weights, trapezoid weights, sub-diagonal, factors
};

struct ChanflowFields { double *U, *V, *W; };
struct ChanflowCFields { const double *U, *V, *W; };

FNO_DEV double cf_wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
// sum over the workgroup (256 threads), the same value in every thread; `red` = 4 doubles of LDS
FNO_DEV double cf_block_sum(double v, double* red) {
  v = cf_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// ---------------------------------------------------------------------------------------------------------------------------
// stage state + divergence + forward transforms
// ---------------------------------------------------------------------------------------------------------------------------
struct ChanflowStageArgs {
  ChanflowCFields X0, F1, Fs;     // F1.U == null: the state is X0 itself; Fs.U == null: one right-hand side
  ChanflowFields out;             // out.U == null: nothing is written (projection of a given state, pressure)
  const double *opV1, *opV2;      // (B, Nx, Nz) wall-normal velocity at the two walls, or null: V's own wall rows
  double ca, cb;                  // dt * a, dt * b
  double2* h;
  int xc;                         // x rows per chunk of the divergence buffer
};

__global__ __launch_bounds__(256) void k_chanflow_stage(ChanflowGeo g, ChanflowTab t, ChanflowStageArgs a) {
  extern __shared__ double cf_lds[];
  const int Nx = g.Nx, Ny = g.Ny, Nz = g.Nz, Nzh = Nz / 2 + 1, DS = Nz + 1;
  const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  double2* Z = (double2*)cf_lds;                       // [Nx][Nzh]
  double2* twx = Z + Nx * Nzh;                         // [Nx]
  double2* twz = twx + Nx;                             // [Nz]
  double* Dc = (double*)(twz + Nz);                    // [xc][DS]
  for (int m = tid; m < Nx; m += 256) twx[m] = ((const double2*)(t.base + t.twx))[m];
  for (int m = tid; m < Nz; m += 256) twz[m] = ((const double2*)(t.base + t.twz))[m];
  const size_t su = (size_t)(Ny + 1) * Nz, sv = (size_t)Ny * Nz;
  const size_t ub = (size_t)b * Nx * su, vb = (size_t)b * Nx * sv, wb = (size_t)b * Nx * Nz;
  const bool comb = a.F1.U != nullptr, two = a.Fs.U != nullptr;
  const double ca = a.ca, cb = a.cb;
  auto val = [&](const double* x0, const double* f1, const double* fs, size_t at) {
    double v = x0[at];
    if (comb) {
      double d = ca * f1[at];
      if (two) d += cb * fs[at];
      v += d;
    }
    return v;
  };
  auto valV = [&](int i, int row, int k) {
    if (a.opV1 && row == 0) return a.opV1[wb + (size_t)i * Nz + k];
    if (a.opV2 && row == Ny - 1) return a.opV2[wb + (size_t)i * Nz + k];
    return val(a.X0.V, a.F1.V, a.Fs.V, vb + i * sv + (size_t)row * Nz + k);
  };
  const double rdx = g.rdx, rdz = g.rdz, ry = g.metrics[j + 1];
  for (int i0 = 0; i0 < Nx; i0 += a.xc) {
    const int rows = min(a.xc, Nx - i0);
    for (int idx = tid; idx < rows * Nz; idx += 256) {
      const int il = idx / Nz, k = idx - il * Nz, i = i0 + il;
      const int ip = (i + 1 == Nx) ? 0 : i + 1, kp = (k + 1 == Nz) ? 0 : k + 1;
      const size_t r1 = (size_t)(j + 1) * Nz;
      const double u = val(a.X0.U, a.F1.U, a.Fs.U, ub + i * su + r1 + k);
      const double up = val(a.X0.U, a.F1.U, a.Fs.U, ub + ip * su + r1 + k);
      const double w = val(a.X0.W, a.F1.W, a.Fs.W, ub + i * su + r1 + k);
      const double wp = val(a.X0.W, a.F1.W, a.Fs.W, ub + i * su + r1 + kp);
      const double v0 = valV(i, j, k), v1 = valV(i, j + 1, k);
      if (a.out.U) {
        double *Uo = a.out.U + ub + i * su, *Wo = a.out.W + ub + i * su, *Vo = a.out.V + vb + i * sv;
        Uo[r1 + k] = u;
        Wo[r1 + k] = w;
        Vo[(size_t)j * Nz + k] = v0;
        if (j == 0) { Uo[k] = -u; Wo[k] = -w; }                                   // ghost rows by reflection
        if (j == Ny - 2) { Uo[r1 + Nz + k] = -u; Wo[r1 + Nz + k] = -w; Vo[r1 + k] = v1; }
      }
      Dc[il * DS + k] = (up - u) * rdx + (v1 - v0) * ry + (wp - w) * rdz;
    }
    __syncthreads();
    for (int o = tid; o < rows * Nzh; o += 256) {
      const int il = o / Nzh, kz = o - il * Nzh;
      const double* d = Dc + il * DS;
      double re = 0.0, im = 0.0;
      for (int k = 0, m = 0; k < Nz; ++k) {
        const double2 w = twz[m];
        re += d[k] * w.x;
        im += d[k] * w.y;
        m += kz;
        if (m >= Nz) m -= Nz;
      }
      Z[(i0 + il) * Nzh + kz] = make_double2(re, im);
    }
    __syncthreads();
  }
  double2* h = a.h + ((size_t)b * (Ny - 1) + j) * ((size_t)Nx * Nzh);
  for (int o = tid; o < Nx * Nzh; o += 256) {
    const int kx = o / Nzh, kz = o - kx * Nzh;
    double re = 0.0, im = 0.0;
    for (int i = 0, m = 0; i < Nx; ++i) {
      const double2 z = Z[i * Nzh + kz], w = twx[m];
      re += z.x * w.x - z.y * w.y;
      im += z.x * w.y + z.y * w.x;
      m += kx;
      if (m >= Nx) m -= Nx;
    }
    h[o] = make_double2(re, im);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// tridiagonal solves: d'[j] = (r[j] - sub[j] d'[j-1]) rp[j];  x[j] = d'[j] - cp[j] x[j+1]
// factors: [tile][row][32 columns] pairs (rp, cp); padded columns carry (1, 0) and are neither loaded nor stored
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_chanflow_solve(int n /* Ny-1 */, int ncol, ChanflowTab t, double2* h) {
  extern __shared__ double cf_lds[];
  const int tile = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int c0 = tile * kCfTile, cols = min(kCfTile, ncol - c0);
  double2* T = (double2*)cf_lds;                        // [n][32]: row j = (re, im) of 32 columns, as in memory
  double2* Fc = T + n * kCfTile;                        // [n][32]: (rp, cp) of the tile, as in the table
  double* S = (double*)(Fc + n * kCfTile);              // [n]: sub-diagonal
  double2* hb = h + (size_t)b * n * ncol + c0;
  const double2* fac = (const double2*)(t.base + t.fac) + (size_t)tile * n * kCfTile;
  // all 256 threads stage the tile, four elements per thread and pass: the eight loads of a group are issued before its first
  // store, from clamped addresses (a padded column re-reads the tile's last live one, a group past the end the last element)
  const int N = n * kCfTile;
  for (int base = tid; base < N; base += 4 * 256) {
    double2 v[4], f[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int idx = min(base + u * 256, N - 1), j = idx >> 5, c = idx & 31;
      v[u] = hb[(size_t)j * ncol + min(c, cols - 1)];
      f[u] = fac[idx];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int idx = base + u * 256;
      if (idx < N) {
        T[idx] = ((idx & 31) < cols) ? v[u] : make_double2(0.0, 0.0);
        Fc[idx] = f[u];
      }
    }
  }
  for (int j = tid; j < n; j += 256) S[j] = t.base[t.sub + j];
  __syncthreads();
  if (tid < 64) {                                        // lane = one double of a row: 64 consecutive 8-byte words per step
    double* Td = (double*)T;
    const double2* f = Fc + (tid >> 1);
    double d = 0.0;
#pragma unroll 4
    for (int j = 0; j < n; ++j) {
      d = (Td[j * 64 + tid] - S[j] * d) * f[j * kCfTile].x;
      Td[j * 64 + tid] = d;
    }
    double x = 0.0;
#pragma unroll 4
    for (int j = n - 1; j >= 0; --j) {
      x = Td[j * 64 + tid] - f[j * kCfTile].y * x;
      Td[j * 64 + tid] = x;
    }
  }
  __syncthreads();
  for (int idx = tid; idx < n * kCfTile; idx += 256) {
    const int j = idx >> 5, c = idx & 31;
    if (c < cols) hb[(size_t)j * ncol + c] = T[idx];
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// inverse transforms: p = Re ifft_z ifft_x (cA A + cB B) for one plane, handed row by row to `apply(i, k, p, p_xm, p_zm)`
// (p_xm = p[i-1][k], p_zm = p[i][k-1]).  LDS: Y [Nx][Nzh] complex, twiddles, weights, Pc [(xc+1)][Nz+1].
// ---------------------------------------------------------------------------------------------------------------------------
template <typename Apply>
FNO_DEV void cf_inverse_plane(int Nx, int Nz, int xc, const ChanflowTab& t, double* lds, const double2* A, const double2* B,
                              double cA, double cB, Apply apply) {
  const int Nzh = Nz / 2 + 1, DS = Nz + 1, tid = threadIdx.x;
  double2* Y = (double2*)lds;
  double2* twx = Y + Nx * Nzh;
  double2* twz = twx + Nx;
  double* wgt = (double*)(twz + Nz);                   // [Nzh] rounded up to even
  double* Pc = wgt + ((Nzh + 1) & ~1);
  __syncthreads();                                      // the previous plane's Pc and Y are free
  for (int m = tid; m < Nx; m += 256) twx[m] = ((const double2*)(t.base + t.twx))[m];
  for (int m = tid; m < Nz; m += 256) twz[m] = ((const double2*)(t.base + t.twz))[m];
  for (int m = tid; m < Nzh; m += 256) wgt[m] = t.base[t.wgt + m];
  __syncthreads();
  for (int o = tid; o < Nx * Nzh; o += 256) {           // x inverse, spectra straight from global (L2); conj twiddles
    const int i = o / Nzh, kz = o - i * Nzh;
    double re = 0.0, im = 0.0;
    int m = 0;
    for (int kx = 0; kx < Nx; ++kx) {
      double2 s = A[kx * Nzh + kz];
      s.x *= cA; s.y *= cA;
      if (B) { const double2 q = B[kx * Nzh + kz]; s.x += cB * q.x; s.y += cB * q.y; }
      const double2 w = twx[m];
      re += s.x * w.x + s.y * w.y;
      im += s.y * w.x - s.x * w.y;
      m += i;
      if (m >= Nx) m -= Nx;
    }
    Y[o] = make_double2(re, im);
  }
  __syncthreads();
  const double scale = 1.0 / ((double)Nx * (double)Nz);
  for (int i0 = 0; i0 < Nx; i0 += xc) {
    const int rows = min(xc, Nx - i0);
    for (int idx = tid; idx < (rows + 1) * Nz; idx += 256) {       // local row 0 is the halo i0 - 1
      const int il = idx / Nz, k = idx - il * Nz;
      int i = i0 + il - 1;
      if (i < 0) i += Nx;
      const double2* y = Y + i * Nzh;
      double p = 0.0;
      for (int kz = 0, m = 0; kz < Nzh; ++kz) {
        const double2 w = twz[m];
        p += wgt[kz] * (y[kz].x * w.x + y[kz].y * w.y);
        m += k;
        if (m >= Nz) m -= Nz;
      }
      Pc[il * DS + k] = p * scale;
    }
    __syncthreads();
    for (int idx = tid; idx < rows * Nz; idx += 256) {
      const int il = idx / Nz, k = idx - il * Nz, km = k ? k - 1 : Nz - 1;
      apply(i0 + il, k, Pc[(il + 1) * DS + k], Pc[il * DS + k], Pc[(il + 1) * DS + km]);
    }
    __syncthreads();
  }
}

struct ChanflowCorrectArgs {
  ChanflowCFields in;
  ChanflowFields out;             // may alias `in` (each workgroup reads only what it writes)
  const double2* ph;
  double* rowsum;                 // [B][Ny-1] xz-sums of the corrected U rows 1..Ny-1, or null
  int xc;
};

__global__ __launch_bounds__(256) void k_chanflow_correct(ChanflowGeo g, ChanflowTab t, ChanflowCorrectArgs a) {
  extern __shared__ double cf_lds[];
  __shared__ double red[4];
  const int Nx = g.Nx, Ny = g.Ny, Nz = g.Nz, Nzh = Nz / 2 + 1, MP = Ny + 2;
  const int j = blockIdx.x, b = blockIdx.y;
  const size_t su = (size_t)(Ny + 1) * Nz, sv = (size_t)Ny * Nz, pl = (size_t)Nx * Nzh;
  const size_t ub = (size_t)b * Nx * su, vb = (size_t)b * Nx * sv;
  const double2* ph = a.ph + ((size_t)b * (Ny - 1) + j) * pl;
  const double rdx = g.rdx, rdz = g.rdz;
  const size_t r1 = (size_t)(j + 1) * Nz;
  double acc = 0.0;
  cf_inverse_plane(Nx, Nz, a.xc, t, cf_lds, ph, nullptr, 1.0, 0.0, [&](int i, int k, double p, double pxm, double pzm) {
    const size_t at = ub + i * su + r1 + k;
    const double u = a.in.U[at] - (p - pxm) * rdx, w = a.in.W[at] - (p - pzm) * rdz;
    a.out.U[at] = u;
    a.out.W[at] = w;
    if (j == 0) { a.out.U[at - Nz] = -u; a.out.W[at - Nz] = -w; }
    if (j == Ny - 2) { a.out.U[at + Nz] = -u; a.out.W[at + Nz] = -w; }
    acc += u;
  });
  if (a.rowsum) {
    acc = cf_block_sum(acc, red);
    if (threadIdx.x == 0) a.rowsum[(size_t)b * (Ny - 1) + j] = acc;
  }
  if (j >= 1) {                   // V rows 1..Ny-2: gradient between planes j-1 and j, one inverse of the difference
    const double rm = g.metrics[MP + j];
    cf_inverse_plane(Nx, Nz, a.xc, t, cf_lds, ph, ph - pl, 1.0, -1.0, [&](int i, int k, double p, double, double) {
      const size_t at = vb + i * sv + (size_t)j * Nz + k;
      a.out.V[at] = a.in.V[at] - p * rm;
    });
  }
  if (a.out.V != a.in.V && (j == 0 || j == Ny - 2)) {   // the wall rows keep the wall condition the stage kernel wrote
    const size_t row = (j == 0) ? 0 : (size_t)(Ny - 1) * Nz;
    for (int idx = threadIdx.x; idx < Nx * Nz; idx += 256) {
      const size_t at = vb + (idx / Nz) * sv + row + idx % Nz;
      a.out.V[at] = a.in.V[at];
    }
  }
}

// p1 = -(P[0] + P[1]) / 2, p2 = -(P[Ny-2] + P[Ny-3]) / 2 (B, Nx, Nz); blocks 2.. write plane blockIdx.x - 2 of P (B, Nx, Ny-1, Nz)
__global__ __launch_bounds__(256) void k_chanflow_pressure(ChanflowGeo g, ChanflowTab t, const double2* phat, double* p1,
                                                           double* p2, double* P, int xc) {
  extern __shared__ double cf_lds[];
  const int Nx = g.Nx, Ny = g.Ny, Nz = g.Nz, Nzh = Nz / 2 + 1, n = Ny - 1;
  const int r = blockIdx.x, b = blockIdx.y;
  const size_t pl = (size_t)Nx * Nzh;
  const double2* ph = phat + (size_t)b * n * pl;
  if (r < 2) {
    const int ja = r ? n - 1 : 0, jb = r ? n - 2 : 1;
    double* dst = (r ? p2 : p1) + (size_t)b * Nx * Nz;
    cf_inverse_plane(Nx, Nz, xc, t, cf_lds, ph + ja * pl, ph + jb * pl, -0.5, -0.5,
                     [&](int i, int k, double p, double, double) { dst[(size_t)i * Nz + k] = p; });
  } else {
    const int j = r - 2;
    double* dst = P + (size_t)b * Nx * n * Nz + (size_t)j * Nz;
    cf_inverse_plane(Nx, Nz, xc, t, cf_lds, ph + j * pl, nullptr, 1.0, 0.0,
                     [&](int i, int k, double p, double, double) { dst[(size_t)i * n * Nz + k] = p; });
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// bulk velocity (calculate_meanU :249-259) from the row sums, then U[:, 1:-1] += dPdx_new / 2 and the dPdx update (:575-579)
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_chanflow_bulk(ChanflowGeo g, ChanflowTab t, const double* rowsum, const double* meanU0,
                                                       double dt, double* U, double* dpdx) {
  __shared__ double shift;
  const int Nx = g.Nx, Ny = g.Ny, Nz = g.Nz, i = blockIdx.x, b = blockIdx.y;
  if (threadIdx.x == 0) {
    const double* rs = rowsum + (size_t)b * (Ny - 1);
    double m = 0.0;
    for (int j = 0; j < Ny - 1; ++j) m += rs[j] * t.base[t.trap + j];
    shift = meanU0[b] - m;                             // dPdx_new / 2 = meanU0 - meanU_now
  }
  __syncthreads();
  const double c = shift;
  double* u = U + ((size_t)b * Nx + i) * (size_t)(Ny + 1) * Nz + Nz;
  for (int idx = threadIdx.x; idx < (Ny - 1) * Nz; idx += 256) u[idx] += c;
  if (i == 0 && threadIdx.x == 0) dpdx[b] = 0.5 * (dpdx[b] + 2.0 * c / dt);
}

// ---------------------------------------------------------------------------------------------------------------------------
// diagnostics: out[b][12] = sum(div), mean|U|, mean|V|, mean|W|, ||U||, ||V||, ||W||, |mean wall shear stress|, bulk velocity,
// mean(p2), finite-difference dPdx of p2, mean wall shear stress (signed); the p2 entries are 0 when p2 is null
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_chanflow_diag(ChanflowGeo g, ChanflowTab t, ChanflowCFields x, const double* p2,
                                                       double* out) {
  __shared__ double red[4];
  const int Nx = g.Nx, Ny = g.Ny, Nz = g.Nz, b = blockIdx.x, tid = threadIdx.x;
  const size_t su = (size_t)(Ny + 1) * Nz, sv = (size_t)Ny * Nz;
  const double *U = x.U + (size_t)b * Nx * su, *V = x.V + (size_t)b * Nx * sv, *W = x.W + (size_t)b * Nx * su;
  double s[11];
  for (int q = 0; q < 11; ++q) s[q] = 0.0;
  for (size_t idx = tid; idx < (size_t)Nx * su; idx += 256) {
    const double u = U[idx], w = W[idx];
    s[1] += fabs(u); s[4] += u * u;
    s[3] += fabs(w); s[6] += w * w;
  }
  for (size_t idx = tid; idx < (size_t)Nx * sv; idx += 256) {
    const double v = V[idx];
    s[2] += fabs(v); s[5] += v * v;
  }
  const int npl = Nx * Nz;
  for (int idx = tid; idx < (Ny - 1) * npl; idx += 256) {       // divergence (:186-194) and the bulk-velocity profile
    const int j = idx / npl, r = idx - j * npl, i = r / Nz, k = r - i * Nz;
    const int ip = (i + 1 == Nx) ? 0 : i + 1, kp = (k + 1 == Nz) ? 0 : k + 1;
    const size_t r1 = (size_t)(j + 1) * Nz;
    const double u = U[i * su + r1 + k];
    s[0] += (U[ip * su + r1 + k] - u) * g.rdx + (V[i * sv + r1 + k] - V[i * sv + r1 - Nz + k]) * g.metrics[j + 1] +
            (W[i * su + r1 + kp] - W[i * su + r1 + k]) * g.rdz;
    s[8] += u * t.base[t.trap + j];
  }
  for (int r = tid; r < npl; r += 256) {                        // wall shear stress (:292-303): -u v + nu dU/dy at the top wall
    const int i = r / Nz, k = r - i * Nz;
    const double* u = U + i * su + k;
    s[7] += -u[(size_t)Ny * Nz] * V[i * sv + (size_t)(Ny - 1) * Nz + k] +
            g.nu * (u[(size_t)(Ny - 1) * Nz] - u[(size_t)(Ny - 2) * Nz]) * g.metrics[Ny - 1];
    if (p2) {
      const double* p = p2 + (size_t)b * npl;
      s[9] += p[r];
      if (i + 1 < Nx) s[10] += fabs((p[r + Nz] - p[r]) * g.rdx);
    }
  }
  for (int q = 0; q < 11; ++q) s[q] = cf_block_sum(s[q], red);
  if (tid == 0) {
    double* o = out + (size_t)b * kCfDiag;
    const double nu_ = (double)Nx * su, nv = (double)Nx * sv;
    o[0] = s[0];
    o[1] = s[1] / nu_; o[2] = s[2] / nv; o[3] = s[3] / nu_;
    o[4] = sqrt(s[4]); o[5] = sqrt(s[5]); o[6] = sqrt(s[6]);
    o[7] = fabs(s[7] / npl);
    o[8] = s[8];
    o[9] = s[9] / npl;
    o[10] = (Nx > 1) ? fabs(s[10] / Nz / (Nx - 1)) : 0.0;
    o[11] = s[7] / npl;
  }
}
