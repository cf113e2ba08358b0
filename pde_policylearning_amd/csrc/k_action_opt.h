// The optimal-observer policy's inner loop on the device (reference: run_control.py:186-224): Adam on the upper-wall action
// itself, through the trained full-field observer.  Per environment b, with S = std + eps and a the float32 action:
//
//   k_act_begin      a = float(opV2_0);  x = float((double(a) - mean) / S)            the leaf and the first observer input
//   k_act_obj_part   workgroup (c, b): sum of field^2 over chunk c of the P * plane predicted points, field = double(y) * S + mean
//                    (product and sum rounded separately, as NormalizerGivenMeanStd.decode on float64), and the sum of
//                    double(a)^2 over the same chunk of the plane: two doubles per workgroup into `ws`
//   k_act_obj_dy     workgroup (c, b) adds the partials of environment b in a fixed order (every workgroup of b the same
//                    order, so the same bits), nf = sqrt(sum field^2), na = sqrt(sum a^2); dy = float(field / nf * S), 0 where
//                    nf == 0 (torch.norm's subgradient); workgroup c = 0 writes parts[b] = {nf + reg * na, nf, na}
//   k_act_update     g = float(double(dx) / S + reg * double(a) / na) (second term 0 where na == 0), torch.optim.Adam's float32
//                    step on (a, g) with k_adam's arithmetic, then x = float((double(a) - mean) / S) for the next epoch.
//                    first != 0 (step 1): the moments are initialised without being read
//   k_act_finish     opV2 = double(a) - the environment's own plane mean (run_control.py:223): one workgroup per environment,
//                    a fixed-order sum as k_ctrl_decode's
// No atomics anywhere: every sum has one order, whatever the batch size and the position in it.
#pragma once
#include <hip/hip_runtime.h>

#include "fno_dev.h"
#include "k_chanflow_step.h"

static const int kActChunk = 1024;        // points per workgroup of the objective: 256 threads, four trips

struct ActStats {
  const double *mean, *sd;                // (plane,)
  double eps;
};

__global__ __launch_bounds__(256) void k_act_begin(size_t plane, const double* v0, ActStats s, float* a, float* x, size_t x_stride) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= plane) return;
  const size_t b = blockIdx.y;
  const float av = (float)v0[b * plane + i];
  a[b * plane + i] = av;
  x[b * x_stride + i] = (float)(((double)av - s.mean[i]) / (s.sd[i] + s.eps));
}

FNO_DEV double act_field(float y, double S, double mean) {
#pragma clang fp contract(off)
  const double t = (double)y * S;
  return t + mean;
}

struct ActObjArgs {
  const float *y, *a;                     // (B, P, plane), (B, plane)
  ActStats s;
  size_t plane, total;                    // total = P * plane
  int nchunk;                             // ceil(total / kActChunk)
  double reg;
  double *ws, *parts;                     // (B, nchunk, 2), (B, 3)
  float* dy;                              // (B, P, plane)
};

__global__ __launch_bounds__(256) void k_act_obj_part(ActObjArgs o) {
  __shared__ double red[4];
  const size_t b = blockIdx.y, base = (size_t)blockIdx.x * kActChunk;
  const float *y = o.y + b * o.total, *a = o.a + b * o.plane;
  double sf = 0.0, sa = 0.0;
#pragma unroll
  for (int k = 0; k < kActChunk / 256; ++k) {
    const size_t e = base + (size_t)k * 256 + threadIdx.x;
    if (e < o.total) {
      const size_t i = e % o.plane;
      const double f = act_field(y[e], o.s.sd[i] + o.s.eps, o.s.mean[i]);
      sf += f * f;
    }
    if (e < o.plane) {
      const double v = (double)a[e];
      sa += v * v;
    }
  }
  sf = cf_block_sum(sf, red);
  sa = cf_block_sum(sa, red);
  if (threadIdx.x == 0) {
    double* w = o.ws + (b * o.nchunk + blockIdx.x) * 2;
    w[0] = sf;
    w[1] = sa;
  }
}

__global__ __launch_bounds__(256) void k_act_obj_dy(ActObjArgs o) {
  __shared__ double red[4];
  const size_t b = blockIdx.y, base = (size_t)blockIdx.x * kActChunk;
  const double* w = o.ws + b * o.nchunk * 2;
  double sf = 0.0, sa = 0.0;
  for (int c = threadIdx.x; c < o.nchunk; c += 256) {
    sf += w[2 * c];
    sa += w[2 * c + 1];
  }
  const double nf = sqrt(cf_block_sum(sf, red)), na = sqrt(cf_block_sum(sa, red));
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double* p = o.parts + b * 3;
    p[0] = nf + o.reg * na;
    p[1] = nf;
    p[2] = na;
  }
  const float* y = o.y + b * o.total;
  float* dy = o.dy + b * o.total;
#pragma unroll
  for (int k = 0; k < kActChunk / 256; ++k) {
    const size_t e = base + (size_t)k * 256 + threadIdx.x;
    if (e < o.total) {
      const size_t i = e % o.plane;
      const double S = o.s.sd[i] + o.s.eps;
      dy[e] = nf > 0.0 ? (float)(act_field(y[e], S, o.s.mean[i]) / nf * S) : 0.0f;
    }
  }
}

struct ActUpdateArgs {
  const float* dx;                        // (B, plane): dL/dx of the observer given dy
  const double* parts;                    // (B, 3)
  ActStats s;
  size_t plane, x_stride;
  double reg;
  float beta2, eps, step_size, bc2_sqrt, omb1, omb2;      // k_adam's scalars (fno_adam_scalars, adam_hyper)
  int first;
  float *a, *m, *v, *x;
};

__global__ __launch_bounds__(256) void k_act_update(ActUpdateArgs u) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= u.plane) return;
  const size_t b = blockIdx.y, at = b * u.plane + i;
  const double S = u.s.sd[i] + u.s.eps, na = u.parts[b * 3 + 2];
  float p = u.a[at];
  const float g = (float)((double)u.dx[at] / S + (na > 0.0 ? u.reg * (double)p / na : 0.0));
  float m = u.first ? 0.0f : u.m[at], v = u.first ? 0.0f : u.v[at];
  m = fmaf(g - m, u.omb1, m);
  v = fmaf(g * g, u.omb2, u.beta2 * v);
  const float denom = sqrtf(v) / u.bc2_sqrt + u.eps;
  p = fmaf(-u.step_size, m / denom, p);
  u.a[at] = p;
  u.m[at] = m;
  u.v[at] = v;
  u.x[b * u.x_stride + i] = (float)(((double)p - u.s.mean[i]) / S);
}

__global__ __launch_bounds__(256) void k_act_finish(size_t plane, const float* a, double* opV2) {
  __shared__ double red[4];
  const size_t b = blockIdx.x;
  const float* ab = a + b * plane;
  double* o = opV2 + b * plane;
  double acc = 0.0;
  for (size_t i = threadIdx.x; i < plane; i += 256) acc += (double)ab[i];
  const double m = cf_block_sum(acc, red) / (double)plane;
  for (size_t i = threadIdx.x; i < plane; i += 256) o[i] = (double)ab[i] - m;
}
