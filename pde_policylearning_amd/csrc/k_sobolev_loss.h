// Sobolev (H1) and L2 training losses of neuralop: LpLoss (p = 2) and H1Loss, neuralop/training/losses.py:62-277, forward and
// backward.  x, y (planes, n0, n1, n2) float32 contiguous, n2 innermost; a d-dimensional grid fills the LAST d axes and the
// leading ones have extent 1.  A plane is one (batch, channel) index.  With e = x - y and, on every grid axis k,
//   D_k v[i] = (v[i+1] - v[i-1]) / (2 h_k), indices mod n_k (torch.roll);
//   fixed (non-periodic) axis: D_k v[0] = (v[1] - v[0]) / h_k, D_k v[n-1] = (v[n-1] - v[n-2]) / h_k, interior rows unchanged,
// a plane has   num = sum e^2 + sum_k sum (D_k e)^2,   den = sum y^2 + sum_k sum (D_k y)^2   (order 0: without the D terms)
//   relative: value = sqrt(num / den)          absolute: value = sqrt(vol num), vol = prod h_k
//   dx = s (e + sum_k D_k^T D_k e),  s = g / sqrt(num den)  or  g sqrt(vol) / sqrt(num);  s = 0 for a plane with num == 0
// (the reference's autograd gives NaN there).
//
// The adjoint is COMPOSED from the rules, never written as a five-point formula, so that extents 2, 3 and 4 (where i +- 1 and
// i +- 2 coincide or wrap onto each other) and fixed ends within three rows of each other need no case of their own:
//   periodic: (D^T r)[i] = (r[i-1] - r[i+1]) / (2h) with r[j] = (e[j+1] - e[j-1]) / (2h); the tile is loaded with wrapped
//             indices, so the LDS offsets -2 .. +2 of a cell ARE e[(i + o) mod n];
//   fixed:    the same with r[0] and r[n-1] taken as zero, then  -r[0]/h at 0, +r[0]/h at 1, +r[n-1]/h at n-1, -r[n-1]/h at
//             n-2 with r[0] = (e[1] - e[0]) / h, r[n-1] = (e[n-1] - e[n-2]) / h - four independent conditions, several of
//             which hold at once for n <= 3.
//
// Tiling.  One workgroup owns one tile of one plane (SOB_T*: cells per axis) and keeps e (forward: and y) in LDS with a halo
// of 1 (forward) or 2 (backward) cells on the grid axes, wrapped at the plane's edge.  Only the plus-shaped part of the halo
// is loaded: a difference runs along one axis.  Order 0 (Lp) has no halo and no LDS: the plane is taken flat, SOB_T0 cells per
// workgroup, straight from global memory.
//   forward : squares in float32 per cell (e^2 + sum_k (D_k e)^2: at most four terms), float64 across cells, one (num, den)
//             pair of float64 partials per workgroup.
//   finish  : a segment of `seg` lanes (a power of two that depends on the tiles per plane alone) adds one plane's partials in
//             a fixed order, keeps (num, den) in float64 for the backward and writes the plane's value; with a batch reduction
//             one workgroup per channel adds the values of its planes over b in a fixed order (sum or mean).
//   backward: one launch, every cell of dx written once, lanes along the innermost axis.
// Fixed order and no atomics: bitwise repeatable, and a plane sees the same operations whatever else is in the call.
#pragma once
#include "k_burgers_loss.h"

constexpr int SOB_NT = 256;              // threads (4 waves: burgers_block_sum)
constexpr int SOB_T0 = 2048;             // order 0: cells of the flattened plane per workgroup
constexpr int SOB_T1D_X = 1024;          // d = 1 tile
constexpr int SOB_T2D_Y = 16;            // d = 2 tile: 16 rows of 64
constexpr int SOB_T2D_X = 64;
constexpr int SOB_T3D_Z = 4;             // d = 3 tile: 4 x 8 rows of 64 (first, second, last grid axis); 8 x 8 x 64 measured 20 % slower
constexpr int SOB_T3D_Y = 8;
constexpr int SOB_T3D_X = 64;
enum { SOB_REDUCE_NONE = 0, SOB_REDUCE_SUM = 1, SOB_REDUCE_MEAN = 2 };

template <int D, int ORDER> struct SobTile;      // cells per internal axis (0, 1, 2)
template <> struct SobTile<1, 0> { static constexpr int T0 = 1, T1 = 1, T2 = SOB_T0; };
template <> struct SobTile<1, 1> { static constexpr int T0 = 1, T1 = 1, T2 = SOB_T1D_X; };
template <> struct SobTile<2, 1> { static constexpr int T0 = 1, T1 = SOB_T2D_Y, T2 = SOB_T2D_X; };
template <> struct SobTile<3, 1> { static constexpr int T0 = SOB_T3D_Z, T1 = SOB_T3D_Y, T2 = SOB_T3D_X; };

struct SobolevArgs {
  const float* x;        // (planes, n0, n1, n2)
  const float* y;
  double* part;          // workspace: (planes * per, 2) sums of a tile
  double* stats;         // workspace: (planes, 2) num, den
  const float* grad;     // backward: (planes) or, with a batch reduction, (channels)
  float* dx;             // backward: (planes, n0, n1, n2)
  int n[3], c[3];        // extents and tiles per axis
  int per;               // tiles per plane
  int fix[3];            // 1: the axis is not periodic
  float inv2h[3], invh[3];
  int relative, reduce, channels, batch;
  double vol;
};

FNO_DEV int sob_wrap(int v, int n) { return v < 0 ? v + n : (v >= n ? v - n : v); }      // v in [-2, n + 1], n >= 2

// D v at the cell of LDS index idx, global index g of an axis with LDS stride st
FNO_DEV float sob_diff(const float* s, int idx, int st, int g, int n, int fix, float inv2h, float invh) {
  if (fix && g == 0) return (s[idx + st] - s[idx]) * invh;
  if (fix && g == n - 1) return (s[idx] - s[idx - st]) * invh;
  return (s[idx + st] - s[idx - st]) * inv2h;
}

// (D^T D e) at the cell, composed as the header states
FNO_DEV float sob_dtd(const float* s, int idx, int st, int g, int n, int fix, float inv2h, float invh) {
  const float c = s[idx];
  float rm = (c - s[idx - 2 * st]) * inv2h;       // r[g - 1]
  float rp = (s[idx + 2 * st] - c) * inv2h;       // r[g + 1]
  if (fix) {
    const int jm = g == 0 ? n - 1 : g - 1, jp = g == n - 1 ? 0 : g + 1;
    if (jm == 0 || jm == n - 1) rm = 0.f;
    if (jp == 0 || jp == n - 1) rp = 0.f;
  }
  float v = (rm - rp) * inv2h;
  if (fix) {
    if (g <= 1) {                                 // r[0] = (e[1] - e[0]) / h: -r[0]/h at 0, +r[0]/h at 1
      const float r0 = (g == 0 ? s[idx + st] - c : c - s[idx - st]) * invh;
      v += (g == 0 ? -r0 : r0) * invh;
    }
    if (g >= n - 2) {                             // r[n-1] = (e[n-1] - e[n-2]) / h: +r[n-1]/h at n-1, -r[n-1]/h at n-2
      const float rn = (g == n - 1 ? c - s[idx - st] : s[idx + st] - c) * invh;
      v += (g == n - 1 ? rn : -rn) * invh;
    }
  }
  return v;
}

// the tile of this workgroup: plane p, origin o, owned extents e
struct SobOwn { int p, o[3], e[3]; size_t base; };
template <int T0, int T1, int T2>
FNO_DEV SobOwn sob_own(const SobolevArgs& a) {
  SobOwn w;
  w.p = blockIdx.x / a.per;
  const int tile = blockIdx.x % a.per;
  w.o[2] = (tile % a.c[2]) * T2;
  w.o[1] = ((tile / a.c[2]) % a.c[1]) * T1;
  w.o[0] = (tile / (a.c[2] * a.c[1])) * T0;
  w.e[0] = min(T0, a.n[0] - w.o[0]);
  w.e[1] = min(T1, a.n[1] - w.o[1]);
  w.e[2] = min(T2, a.n[2] - w.o[2]);
  w.base = (size_t)w.p * (size_t)a.n[0] * (size_t)a.n[1] * (size_t)a.n[2];
  return w;
}

// e = x - y (and y when Ys is given) of the tile and the plus-shaped halo of H cells on the grid axes, wrapped
template <int D, int H, int T0, int T1, int T2>
FNO_DEV void sob_load(const SobolevArgs& a, const SobOwn& w, float* Es, float* Ys) {
  constexpr int H0 = D >= 3 ? H : 0, H1 = D >= 2 ? H : 0, H2 = H;
  constexpr int W0 = T0 + 2 * H0, W1 = T1 + 2 * H1, W2 = T2 + 2 * H2;
  const float* xp = a.x + w.base;
  const float* yp = a.y + w.base;
  for (int idx = threadIdx.x; idx < W0 * W1 * W2; idx += SOB_NT) {
    const int l2 = idx % W2 - H2, l1 = (idx / W2) % W1 - H1, l0 = idx / (W2 * W1) - H0;
    if (l0 >= w.e[0] + H0 || l1 >= w.e[1] + H1 || l2 >= w.e[2] + H2) continue;
    const int outside = (l0 < 0 || l0 >= w.e[0]) + (l1 < 0 || l1 >= w.e[1]) + (l2 < 0 || l2 >= w.e[2]);
    if (outside > 1) continue;
    const int g0 = sob_wrap(w.o[0] + l0, a.n[0]), g1 = sob_wrap(w.o[1] + l1, a.n[1]), g2 = sob_wrap(w.o[2] + l2, a.n[2]);
    const int off = (g0 * a.n[1] + g1) * a.n[2] + g2;
    const float yv = yp[off];
    Es[idx] = xp[off] - yv;
    if (Ys) Ys[idx] = yv;
  }
}

template <int D, int ORDER>
__global__ void __launch_bounds__(SOB_NT) k_sobolev_fwd(SobolevArgs a) {
  using TL = SobTile<D, ORDER>;
  constexpr int T0 = TL::T0, T1 = TL::T1, T2 = TL::T2, H = ORDER ? 1 : 0;
  constexpr int H0 = D >= 3 ? H : 0, H1 = D >= 2 ? H : 0, H2 = H;
  constexpr int W1 = T1 + 2 * H1, W2 = T2 + 2 * H2, LDS = ORDER ? (T0 + 2 * H0) * W1 * W2 : 1;
  __shared__ float Es[LDS];
  __shared__ float Ys[LDS];
  __shared__ double red[SOB_NT / 64];
  const int tid = threadIdx.x;
  const SobOwn w = sob_own<T0, T1, T2>(a);
  double sn = 0.0, sd = 0.0;
  if constexpr (ORDER == 0) {
    const float* xp = a.x + w.base + w.o[2];
    const float* yp = a.y + w.base + w.o[2];
#pragma unroll 4
    for (int i = tid; i < w.e[2]; i += SOB_NT) {
      const float yv = yp[i];
      const double e = (double)(xp[i] - yv), yd = (double)yv;
      sn = fma(e, e, sn);
      sd = fma(yd, yd, sd);
    }
  } else {
    sob_load<D, H, T0, T1, T2>(a, w, Es, Ys);
    __syncthreads();
    for (int c = tid; c < T0 * T1 * T2; c += SOB_NT) {
      const int l2 = c % T2, l1 = (c / T2) % T1, l0 = c / (T2 * T1);
      if (l0 >= w.e[0] || l1 >= w.e[1] || l2 >= w.e[2]) continue;
      const int idx = ((l0 + H0) * W1 + (l1 + H1)) * W2 + (l2 + H2);
      const float e = Es[idx], yv = Ys[idx];
      float se = e * e, sy = yv * yv;
      {
        const int g = w.o[2] + l2;
        const float de = sob_diff(Es, idx, 1, g, a.n[2], a.fix[2], a.inv2h[2], a.invh[2]);
        const float dy = sob_diff(Ys, idx, 1, g, a.n[2], a.fix[2], a.inv2h[2], a.invh[2]);
        se = fmaf(de, de, se);
        sy = fmaf(dy, dy, sy);
      }
      if constexpr (D >= 2) {
        const int g = w.o[1] + l1;
        const float de = sob_diff(Es, idx, W2, g, a.n[1], a.fix[1], a.inv2h[1], a.invh[1]);
        const float dy = sob_diff(Ys, idx, W2, g, a.n[1], a.fix[1], a.inv2h[1], a.invh[1]);
        se = fmaf(de, de, se);
        sy = fmaf(dy, dy, sy);
      }
      if constexpr (D >= 3) {
        const int g = w.o[0] + l0;
        const float de = sob_diff(Es, idx, W1 * W2, g, a.n[0], a.fix[0], a.inv2h[0], a.invh[0]);
        const float dy = sob_diff(Ys, idx, W1 * W2, g, a.n[0], a.fix[0], a.inv2h[0], a.invh[0]);
        se = fmaf(de, de, se);
        sy = fmaf(dy, dy, sy);
      }
      sn += (double)se;
      sd += (double)sy;
    }
  }
  sn = burgers_block_sum(sn, red, tid);
  __syncthreads();
  sd = burgers_block_sum(sd, red, tid);
  if (tid == 0) {
    double* o = a.part + (size_t)blockIdx.x * 2;
    o[0] = sn; o[1] = sd;
  }
}

struct SobolevFinish {
  const double* part;    // (planes * per, 2)
  double* stats;         // (planes, 2)
  float* value;          // (planes)
  float* reduced;        // (channels) or null
  int planes, per;
  int seg;               // lanes per plane: a power of two, at most 64
  int cnt, gstride, jstride;      // workgroup g takes the planes g * gstride + j * jstride, j < cnt
  int relative, reduce, batch;
  double vol;
};

__global__ void __launch_bounds__(SOB_NT) k_sobolev_finish(SobolevFinish a) {
  __shared__ double sh[SOB_NT];
  const int tid = threadIdx.x, W = a.seg, nseg = SOB_NT / W, seg = tid / W, l = tid % W;
  double acc = 0.0;
  for (int j0 = 0; j0 < a.cnt; j0 += nseg) {
    const int j = j0 + seg;
    const long long plane = (long long)blockIdx.x * a.gstride + (long long)j * a.jstride;
    const bool live = j < a.cnt && plane < a.planes;
    double s0 = 0.0, s1 = 0.0;
    if (live) {
      const double* p = a.part + (size_t)plane * a.per * 2;
      for (int t = l; t < a.per; t += W) { s0 += p[2 * t]; s1 += p[2 * t + 1]; }
    }
    for (int off = W >> 1; off > 0; off >>= 1) { s0 += __shfl_xor(s0, off, 64); s1 += __shfl_xor(s1, off, 64); }
    if (live) {
      const double val = a.relative ? sqrt(s0 / s1) : sqrt(a.vol * s0);
      if (l == 0) {
        a.stats[2 * plane] = s0; a.stats[2 * plane + 1] = s1;
        a.value[plane] = (float)val;
      }
      acc += val;
    }
  }
  if (a.reduce == SOB_REDUCE_NONE) return;
  if (l == 0) sh[seg] = acc;
  __syncthreads();
  if (tid < 64) {
    double v = 0.0;
    for (int k = tid; k < nseg; k += 64) v += sh[k];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (tid == 0) a.reduced[blockIdx.x] = (float)(a.reduce == SOB_REDUCE_MEAN ? v / (double)a.batch : v);
  }
}

template <int D, int ORDER>
__global__ void __launch_bounds__(SOB_NT) k_sobolev_bwd(SobolevArgs a) {
  using TL = SobTile<D, ORDER>;
  constexpr int T0 = TL::T0, T1 = TL::T1, T2 = TL::T2, H = ORDER ? 2 : 0;
  constexpr int H0 = D >= 3 ? H : 0, H1 = D >= 2 ? H : 0, H2 = H;
  constexpr int W1 = T1 + 2 * H1, W2 = T2 + 2 * H2, LDS = ORDER ? (T0 + 2 * H0) * W1 * W2 : 1;
  __shared__ float Es[LDS];
  const int tid = threadIdx.x;
  const SobOwn w = sob_own<T0, T1, T2>(a);
  const double num = a.stats[2 * (size_t)w.p], den = a.stats[2 * (size_t)w.p + 1];
  float g = a.reduce == SOB_REDUCE_NONE ? a.grad[w.p] : a.grad[w.p % a.channels];
  if (a.reduce == SOB_REDUCE_MEAN) g = (float)((double)g / (double)a.batch);
  const float s = num > 0.0 ? g * (float)(a.relative ? 1.0 / sqrt(num * den) : sqrt(a.vol) / sqrt(num)) : 0.f;
  float* dp = a.dx + w.base;
  if constexpr (ORDER == 0) {
    const float* xp = a.x + w.base + w.o[2];
    const float* yp = a.y + w.base + w.o[2];
#pragma unroll 4
    for (int i = tid; i < w.e[2]; i += SOB_NT) dp[w.o[2] + i] = s * (xp[i] - yp[i]);
  } else {
    sob_load<D, H, T0, T1, T2>(a, w, Es, nullptr);
    __syncthreads();
    for (int c = tid; c < T0 * T1 * T2; c += SOB_NT) {
      const int l2 = c % T2, l1 = (c / T2) % T1, l0 = c / (T2 * T1);
      if (l0 >= w.e[0] || l1 >= w.e[1] || l2 >= w.e[2]) continue;
      const int idx = ((l0 + H0) * W1 + (l1 + H1)) * W2 + (l2 + H2);
      const int g0 = w.o[0] + l0, g1 = w.o[1] + l1, g2 = w.o[2] + l2;
      float v = Es[idx];
      v += sob_dtd(Es, idx, 1, g2, a.n[2], a.fix[2], a.inv2h[2], a.invh[2]);
      if constexpr (D >= 2) v += sob_dtd(Es, idx, W2, g1, a.n[1], a.fix[1], a.inv2h[1], a.invh[1]);
      if constexpr (D >= 3) v += sob_dtd(Es, idx, W1 * W2, g0, a.n[0], a.fix[0], a.inv2h[0], a.invh[0]);
      dp[(g0 * a.n[1] + g1) * a.n[2] + g2] = s * v;
    }
  }
}
