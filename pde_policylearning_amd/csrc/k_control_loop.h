// Closed-loop control on the device (reference: run_control.py): the two bridges between the fp64 channel-flow state and the
// fp32 observer models, the environment's diagnostics as a two-level reduction, and the running per-point statistics of the
// collected dataset.
//
//   k_ctrl_encode   x = float((p - mean) / (std + eps)), evaluated in fp64 with a true division and rounded once
//                   (NormalizerGivenMeanStd.encode on a float64 tensor, then .float(): run_control.py:139-141), written with a
//                   batch stride: channel 0 of a persistent (B, 3, Nx, Nz) observer input, or the (B, 1, Nx, Nz, 1) RNO input
//   k_ctrl_decode   a = double(y) * (std + eps) + mean, product and sum rounded separately as torch does; then scale, clip,
//                   zero-mean (run_control.py:223); opV1 = 0 (one-sided control, :154).  One workgroup owns a sample, so the
//                   plane mean is a fixed-order sum: no atomics, the same bits at every batch position
//   k_chanflow_diag_part / _diag_finish
//                   the twelve scalars of k_chanflow_diag and dPdx: one workgroup per (wall-normal row, sample) writes eleven
//                   partial sums, one workgroup per sample adds them in a fixed order and writes a row of the caller's log
//   k_ctrl_stats    Welford update of per-point mean and M2 for up to eight fields in one launch
#pragma once
#include <hip/hip_runtime.h>

#include "fno_dev.h"
#include "k_chanflow_step.h"

static const int kCtrlDiagOut = 13;       // doubles per sample written by k_chanflow_diag_finish: kCfDiag and dPdx
static const int kCtrlDiagPart = 11;      // partial sums per (row, sample)
static const int kCtrlStatsMax = 8;       // FNO_CTRL_STATS_MAX

__global__ __launch_bounds__(256) void k_ctrl_encode(size_t plane, const double* p, const double* mean, const double* sd, double eps,
                                                     float* x, size_t x_stride) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= plane) return;
  const size_t b = blockIdx.y;
  x[b * x_stride + i] = (float)((p[b * plane + i] - mean[i]) / (sd[i] + eps));
}

struct CtrlDecodeArgs {
  const float* y;
  size_t y_stride, plane;
  const double *mean, *sd;
  double eps, scale, clip;
  int use_scale, zero_mean;
  double *opV1, *opV2;            // opV1 may be null
};

__global__ __launch_bounds__(256) void k_ctrl_decode(CtrlDecodeArgs a) {
  __shared__ double red[4];
  const size_t b = blockIdx.x, n = a.plane;
  const float* y = a.y + b * a.y_stride;
  double* o = a.opV2 + b * n;
  double acc = 0.0;
  for (size_t i = threadIdx.x; i < n; i += 256) {
    double v;
    {
#pragma clang fp contract(off)
      const double t = (double)y[i] * (a.sd[i] + a.eps);
      v = t + a.mean[i];
    }
    if (a.use_scale) v *= a.scale;
    if (a.clip > 0.0) v = fmin(fmax(v, -a.clip), a.clip);
    o[i] = v;
    acc += v;
    if (a.opV1) a.opV1[b * n + i] = 0.0;
  }
  if (!a.zero_mean) return;       // uniform over the workgroup
  const double m = cf_block_sum(acc, red) / (double)n;
  for (size_t i = threadIdx.x; i < n; i += 256) o[i] -= m;      // every thread re-reads what it wrote itself
}

// ---------------------------------------------------------------------------------------------------------------------------
// diagnostics, first level: workgroup (j, b) sums over wall-normal row j (0..Ny) of sample b
//   part[b][j][0..10] = div, |U|, |V|, |W|, U^2, V^2, W^2, wall shear, bulk-velocity profile, p2, |dp2/dx|
// the wall shear stress belongs to row Ny (it reads U rows Ny-2..Ny and V row Ny-1), the two pressure sums to row 0
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_chanflow_diag_part(ChanflowGeo g, ChanflowTab t, ChanflowCFields x, const double* p2,
                                                            double* part) {
  __shared__ double red[4];
  const int Nx = g.Nx, Ny = g.Ny, Nz = g.Nz, j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const size_t su = (size_t)(Ny + 1) * Nz, sv = (size_t)Ny * Nz;
  const double *U = x.U + (size_t)b * Nx * su, *V = x.V + (size_t)b * Nx * sv, *W = x.W + (size_t)b * Nx * su;
  const int npl = Nx * Nz;
  const size_t r1 = (size_t)j * Nz;
  const bool interior = j >= 1 && j <= Ny - 1;
  const double ry = interior ? g.metrics[j] : 0.0, tw = interior ? t.base[t.trap + j - 1] : 0.0;
  double s[kCtrlDiagPart];
  for (int q = 0; q < kCtrlDiagPart; ++q) s[q] = 0.0;
  for (int r = tid; r < npl; r += 256) {
    const int i = r / Nz, k = r - i * Nz;
    const double u = U[i * su + r1 + k], w = W[i * su + r1 + k];
    s[1] += fabs(u); s[4] += u * u;
    s[3] += fabs(w); s[6] += w * w;
    if (j < Ny) {
      const double v = V[i * sv + r1 + k];
      s[2] += fabs(v); s[5] += v * v;
      if (interior) {
        const int ip = (i + 1 == Nx) ? 0 : i + 1, kp = (k + 1 == Nz) ? 0 : k + 1;
        s[0] += (U[ip * su + r1 + k] - u) * g.rdx + (v - V[i * sv + r1 - Nz + k]) * ry + (W[i * su + r1 + kp] - w) * g.rdz;
        s[8] += u * tw;
      }
    } else {
      const double* uc = U + i * su + k;
      s[7] += -u * V[i * sv + (size_t)(Ny - 1) * Nz + k] +
              g.nu * (uc[(size_t)(Ny - 1) * Nz] - uc[(size_t)(Ny - 2) * Nz]) * g.metrics[Ny - 1];
    }
    if (j == 0 && p2) {
      const double* p = p2 + (size_t)b * npl;
      s[9] += p[r];
      if (i + 1 < Nx) s[10] += fabs((p[r + Nz] - p[r]) * g.rdx);
    }
  }
  for (int q = 0; q < kCtrlDiagPart; ++q) s[q] = cf_block_sum(s[q], red);
  if (tid == 0) {
    double* o = part + ((size_t)b * (Ny + 1) + j) * kCtrlDiagPart;
    for (int q = 0; q < kCtrlDiagPart; ++q) o[q] = s[q];
  }
}

// second level: workgroup b; thread (q, c) adds rows c, c + 16, ... of quantity q, the 16 chunk sums are added in order
__global__ __launch_bounds__(256) void k_chanflow_diag_finish(ChanflowGeo g, const double* part, const double* dpdx, double* out,
                                                              size_t out_stride) {
  __shared__ double sm[16][16];
  const int Nx = g.Nx, Ny = g.Ny, Nz = g.Nz, b = blockIdx.x, q = threadIdx.x & 15, c = threadIdx.x >> 4;
  const double* pb = part + (size_t)b * (Ny + 1) * kCtrlDiagPart;
  double v = 0.0;
  if (q < kCtrlDiagPart)
    for (int j = c; j <= Ny; j += 16) v += pb[(size_t)j * kCtrlDiagPart + q];
  sm[c][q] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s[kCtrlDiagPart];
    for (int k = 0; k < kCtrlDiagPart; ++k) {
      double a = 0.0;
      for (int cc = 0; cc < 16; ++cc) a += sm[cc][k];
      s[k] = a;
    }
    double* o = out + (size_t)b * out_stride;
    const double npl = (double)Nx * Nz, nu_ = npl * (Ny + 1), nv = npl * Ny;
    o[0] = s[0];
    o[1] = s[1] / nu_; o[2] = s[2] / nv; o[3] = s[3] / nu_;
    o[4] = sqrt(s[4]); o[5] = sqrt(s[5]); o[6] = sqrt(s[6]);
    o[7] = fabs(s[7] / npl);
    o[8] = s[8];
    o[9] = s[9] / npl;
    o[10] = (Nx > 1) ? fabs(s[10] / Nz / (Nx - 1)) : 0.0;
    o[11] = s[7] / npl;
    o[12] = dpdx[b];
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// running statistics: mean_n = mean_{n-1} + (x - mean_{n-1}) / n,  M2_n = M2_{n-1} + (x - mean_{n-1}) (x - mean_n)
// the first snapshot (count == 1) initialises mean and M2 without reading them
// ---------------------------------------------------------------------------------------------------------------------------
struct CtrlStatsTab {
  const double* x[kCtrlStatsMax];
  double* mean[kCtrlStatsMax];
  double* m2[kCtrlStatsMax];
  size_t n[kCtrlStatsMax];
};

__global__ __launch_bounds__(256) void k_ctrl_stats(CtrlStatsTab t, double count) {
  const int f = blockIdx.y;
  const double* x = t.x[f];
  double *mean = t.mean[f], *m2 = t.m2[f];
  const size_t n = t.n[f], step = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
    const double v = x[i];
    if (count == 1.0) {
      mean[i] = v;
      m2[i] = 0.0;
    } else {
      const double m0 = mean[i], d = v - m0, m1 = m0 + d / count;
      mean[i] = m1;
      m2[i] += d * (v - m1);
    }
  }
}
