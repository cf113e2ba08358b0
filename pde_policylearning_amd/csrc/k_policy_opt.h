// The optimal-policy-observer policy's glue on the device (reference: run_control.py:162-185): a neural policy maps the raw
// wall pressure to a correction `res` of the opposition-control action a0 and is trained on line through the frozen
// full-field observer.  The two networks run on the engine's existing paths; these three kernels sit between them:
//
//   k_pol_begin      a0 = float(opV2_0);  pin = float(p2)                 the start action and the policy's input, one launch
//   k_pol_compose    x = a0 + res (one float32 add);  opV2 = double(x)    the observer's input (a persistent leaf) and, in the
//                    same pass, the action the loop applies: what the last epoch leaves IS the reference's opV2
//   k_pol_grad       g = float(double(dx) + reg * double(x) / na)         dL/dres, assembled in float64 and rounded once;
//                    na = parts[b][2] of fno_ctrl_action_objective, the second term 0 where na == 0
//
// The objective between compose and grad is fno_ctrl_action_objective (k_action_opt.h) as it stands, called with a := x and
// unit statistics.  Elementwise, no reduction, no atomics: batch-position and run-to-run invariant by construction.
#pragma once
#include <hip/hip_runtime.h>

__global__ __launch_bounds__(256) void k_pol_begin(size_t plane, const double* v0, const double* p2, float* a0, float* pin) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= plane) return;
  const size_t at = (size_t)blockIdx.y * plane + i;
  a0[at] = (float)v0[at];
  pin[at] = (float)p2[at];
}

__global__ __launch_bounds__(256) void k_pol_compose(size_t plane, const float* a0, const float* res, float* x, double* opV2) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= plane) return;
  const size_t at = (size_t)blockIdx.y * plane + i;
  const float v = a0[at] + res[at];
  x[at] = v;
  opV2[at] = (double)v;
}

__global__ __launch_bounds__(256) void k_pol_grad(size_t plane, const float* dx, const float* x, const double* parts, double reg,
                                                  float* g) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= plane) return;
  const size_t b = blockIdx.y, at = b * plane + i;
  const double na = parts[b * 3 + 2];
  const float d = dx[at];
  g[at] = na > 0.0 ? (float)((double)d + reg * (double)x[at] / na) : d;      // (na == 0: dx as it is, the sign of a zero too)
}
