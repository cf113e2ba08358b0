// Spectral Sobolev loss of the original FNO code base: HsLoss, libs/utilities3.py:339-405, forward and backward.
// x, y (B, N, N, C) float32 contiguous, channels LAST (every trailing dimension of the caller's tensor folded into C), N = 32, 64
// or 128.  With e = x - y, E = fft2(e), Y = fft2(y) per (sample, channel) plane and r2 = kx^2 + ky^2 of the ABSOLUTE wave numbers
// |k|, k = [0 .. N/2-1, -N/2 .. -1] (the Nyquist index carries N/2), the terms j = 0, 1, 2 are
//   num_j = w2[j] sum_{kx,ky,c} r2^j |E|^2,   den_j = w2[j] sum r2^j |Y|^2,   w2 = (1, a[0]^2, a[1]^2)
//   ungrouped: v_b = sqrt(sum_j num_j) / sqrt(sum_j den_j)        grouped: v_b = (sum_j sqrt(num_j) / sqrt(den_j)) / divisor
//   dx = Re(ifft2_unnormalised(Wc E)),  Wc = sum_j c_j w2[j] r2^j,  c_j = g_b / sqrt(num den)  or  g_b / (divisor sqrt(num_j den_j));
//   a term (ungrouped: a sample) whose num is exactly zero contributes zero.
//
// One workgroup owns one SLOT of one sample: the channel pair (2s, 2s + 1), packed as one complex plane e_2s + i e_2s+1 (the last
// slot of an odd C has a zero imaginary part).  The weights are real and even in k, so sum W |fft2(e0 + i e1)|^2 is
// sum W |E0|^2 + sum W |E1|^2 (the cross terms of k and -k cancel) and Re / Im of ifft2(Wc fft2(e0 + i e1)) are the two channels'
// gradients: one transform serves two planes, and the two channels of a pair are adjacent in memory.  e is NEVER packed with y:
// near convergence |e| ~ 1e-3 |y| and the rounding of y's spectrum (relative to |y|) would land in e's.  y is transformed on its
// own, after e, through the same LDS grid (kept in registers meanwhile: the plane is read from memory once).
// The transforms are the in-LDS radix-2 FFTs of k_pino_loss.h: forward leaves the spectrum bit-reversed, so r2 is evaluated at the
// bit-reversed position (as pino_mult is) and the inverse takes it back without a reordering pass.
//   plane   : |Z|^2 and its products with r2, r2^2 in float32 per bin, float64 across bins: lanes by xor shuffle, then the waves in
//             index order.  Six float64 sums per slot (r2^j |E|^2, r2^j |Y|^2, without w2), unused terms written as zero.
//   finish  : one workgroup; a thread adds the slots of its samples in slot order, applies w2, keeps (num_j, den_j) in float64 for the
//             backward, writes the sample's value, and the values are added over b in a fixed order (thread-strided, then a tree).
//   backward: one launch, e transformed again, multiplied by the real weight, inverse transform, both channels written.
// Fixed order and no atomics: bitwise repeatable, and a sample sees the same operations whatever else is in the call.
#pragma once
#include "k_pino_loss.h"

enum { HS_REDUCE_NONE = 0, HS_REDUCE_SUM = 1, HS_REDUCE_MEAN = 2 };
constexpr int HS_TERMS = 3;              // |k|^0, |k|^2, |k|^4: the orders that ever enter (utilities3.py:387-402)
constexpr int HS_FINISH_NT = 256;

struct HsArgs {
  const float* x;        // (B, N, N, C)
  const float* y;
  double* part;          // workspace: (B * slots, 2, HS_TERMS) sums of a slot
  const double* stats;   // workspace: (B, 2, HS_TERMS) num_j, den_j            (backward)
  const float* grad;     // backward: (B) without a reduction, else one scalar
  float* dx;             // backward: (B, N, N, C)
  int C, slots, terms, group, reduce, batch;
  double w2[HS_TERMS];
  double divisor;
};

// r2 = kx^2 + ky^2 of the bin that the forward transform leaves at LDS position (p, q)
template <int N>
FNO_DEV float hs_r2(int p, int q) {
  const int ix = brev_n<N>(p), iy = brev_n<N>(q);
  const int kx = min(ix, N - ix), ky = min(iy, N - iy);      // |k|: index N/2 carries N/2
  return (float)(kx * kx + ky * ky);
}

// forward transform of the grid, then out[j] = sum over the bins of r2^j |Z|^2, j < HS_TERMS (zero for j >= terms)
template <int N, int NT>
FNO_DEV void hs_spectrum_sums(float2* G, const float2* tw, double* red, int terms, double* out, int tid) {
  constexpr int P = N + 1, NWV = NT / 64, PPT = N * N / NT;
  const int lane = tid & 63, wave = tid >> 6;
  fft2_grid<N, false, NWV>(G, tw, wave, lane);
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int e = tid + NT * j, p = e / N, q = e % N;
    const float2 v = G[p * P + q];
    const float m = fmaf(v.x, v.x, v.y * v.y);
    const float r2 = hs_r2<N>(p, q);
    s0 += (double)m;
    if (terms > 1) s1 += (double)(r2 * m);
    if (terms > 2) s2 += (double)(r2 * r2 * m);
  }
  for (int off = 32; off > 0; off >>= 1) {
    s0 += __shfl_xor(s0, off, 64); s1 += __shfl_xor(s1, off, 64); s2 += __shfl_xor(s2, off, 64);
  }
  if (lane == 0) { red[wave * HS_TERMS] = s0; red[wave * HS_TERMS + 1] = s1; red[wave * HS_TERMS + 2] = s2; }
  __syncthreads();
  if (tid < HS_TERMS) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < NWV; ++k) t += red[k * HS_TERMS + tid];
    out[tid] = t;
  }
  __syncthreads();      // red and G are free again
}

template <int N>
FNO_DEV void hs_twiddles(float2* tw, int tid, int nt) {
  for (int k = tid; k < N / 2; k += nt) {
    float sn, cs;
    sincospif(-2.0f * (float)k / (float)N, &sn, &cs);      // exact argument (k / N is dyadic)
    tw[k] = make_float2(cs, sn);
  }
}

template <int N>
__global__ void __launch_bounds__(PinoCfg<N>::NT) k_hs_plane_fwd(HsArgs a) {
  constexpr int P = N + 1, NT = PinoCfg<N>::NT, PPT = N * N / NT;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float2* G = reinterpret_cast<float2*>(smem);
  float2* tw = G + N * P;
  double* red = reinterpret_cast<double*>(tw + N / 2);
  const int tid = threadIdx.x;
  const int b = blockIdx.x / a.slots, c0 = 2 * (blockIdx.x % a.slots);
  const bool two = c0 + 1 < a.C;
  const size_t base = (size_t)b * N * N * a.C + c0;
  hs_twiddles<N>(tw, tid, NT);
  float yre[PPT], yim[PPT];
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int e = tid + NT * j;
    const size_t o = base + (size_t)e * a.C;
    const float y0 = a.y[o], x0 = a.x[o];
    const float y1 = two ? a.y[o + 1] : 0.f, x1 = two ? a.x[o + 1] : 0.f;
    G[(e / N) * P + e % N] = make_float2(x0 - y0, x1 - y1);
    yre[j] = y0; yim[j] = y1;
  }
  __syncthreads();
  double* out = a.part + (size_t)blockIdx.x * 2 * HS_TERMS;
  hs_spectrum_sums<N, NT>(G, tw, red, a.terms, out, tid);
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int e = tid + NT * j;
    G[(e / N) * P + e % N] = make_float2(yre[j], yim[j]);
  }
  __syncthreads();
  hs_spectrum_sums<N, NT>(G, tw, red, a.terms, out + HS_TERMS, tid);
}

struct HsFinish {
  const double* part;    // (B * slots, 2, HS_TERMS)
  double* stats;         // (B, 2, HS_TERMS)
  float* value;          // (B)
  float* reduced;        // one scalar, or null without a reduction
  int B, slots, terms, group, reduce;
  double w2[HS_TERMS];
  double divisor;
};

__global__ void __launch_bounds__(HS_FINISH_NT) k_hs_finish(HsFinish a) {
  __shared__ double sh[HS_FINISH_NT];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int b = tid; b < a.B; b += HS_FINISH_NT) {
    double S[2 * HS_TERMS];
#pragma unroll
    for (int t = 0; t < 2 * HS_TERMS; ++t) S[t] = 0.0;
    for (int s = 0; s < a.slots; ++s) {
      const double* p = a.part + ((size_t)b * a.slots + s) * 2 * HS_TERMS;
#pragma unroll
      for (int t = 0; t < 2 * HS_TERMS; ++t) S[t] += p[t];
    }
    double num = 0.0, den = 0.0, grouped = 0.0;
#pragma unroll
    for (int j = 0; j < HS_TERMS; ++j) {
      const bool live = j < a.terms;
      const double nj = live ? a.w2[j] * S[j] : 0.0, dj = live ? a.w2[j] * S[HS_TERMS + j] : 0.0;
      a.stats[(size_t)b * 2 * HS_TERMS + j] = nj;
      a.stats[(size_t)b * 2 * HS_TERMS + HS_TERMS + j] = dj;
      num += nj; den += dj;
      if (live) grouped += sqrt(nj) / sqrt(dj);
    }
    const double v = a.group ? grouped / a.divisor : sqrt(num) / sqrt(den);
    a.value[b] = (float)v;
    acc += v;
  }
  if (a.reduce == HS_REDUCE_NONE) return;
  sh[tid] = acc;
  __syncthreads();
  for (int off = HS_FINISH_NT / 2; off > 0; off >>= 1) {
    if (tid < off) sh[tid] += sh[tid + off];
    __syncthreads();
  }
  if (tid == 0) a.reduced[0] = (float)(a.reduce == HS_REDUCE_MEAN ? sh[0] / (double)a.B : sh[0]);
}

template <int N>
__global__ void __launch_bounds__(PinoCfg<N>::NT) k_hs_plane_bwd(HsArgs a) {
  constexpr int P = N + 1, NT = PinoCfg<N>::NT, NWV = NT / 64, PPT = N * N / NT;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float2* G = reinterpret_cast<float2*>(smem);
  float2* tw = G + N * P;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / a.slots, c0 = 2 * (blockIdx.x % a.slots);
  const bool two = c0 + 1 < a.C;
  const size_t base = (size_t)b * N * N * a.C + c0;
  hs_twiddles<N>(tw, tid, NT);
  // the real weight's coefficients of r2^0, r2^1, r2^2 (uniform over the workgroup), float64 until the last step
  const double* st = a.stats + (size_t)b * 2 * HS_TERMS;
  double g = (double)a.grad[a.reduce == HS_REDUCE_NONE ? b : 0];
  if (a.reduce == HS_REDUCE_MEAN) g /= (double)a.batch;
  float cf[HS_TERMS];
  const double num = (st[0] + st[1]) + st[2], den = (st[HS_TERMS] + st[HS_TERMS + 1]) + st[HS_TERMS + 2];
  const double call = num > 0.0 ? g / sqrt(num * den) : 0.0;
#pragma unroll
  for (int j = 0; j < HS_TERMS; ++j) {
    double c = 0.0;
    if (j < a.terms) {
      if (!a.group) c = call;
      else if (st[j] > 0.0) c = g / (a.divisor * sqrt(st[j] * st[HS_TERMS + j]));
    }
    cf[j] = (float)(c * a.w2[j]);
  }
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int e = tid + NT * j;
    const size_t o = base + (size_t)e * a.C;
    const float e0 = a.x[o] - a.y[o];
    const float e1 = two ? a.x[o + 1] - a.y[o + 1] : 0.f;
    G[(e / N) * P + e % N] = make_float2(e0, e1);
  }
  __syncthreads();
  fft2_grid<N, false, NWV>(G, tw, wave, lane);
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int e = tid + NT * j, p = e / N, q = e % N;
    const float r2 = hs_r2<N>(p, q);
    const float w = fmaf(r2, fmaf(r2, cf[2], cf[1]), cf[0]);
    const float2 v = G[p * P + q];
    G[p * P + q] = make_float2(w * v.x, w * v.y);
  }
  __syncthreads();
  fft2_grid<N, true, NWV>(G, tw, wave, lane);
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int e = tid + NT * j;
    const size_t o = base + (size_t)e * a.C;
    const float2 v = G[(e / N) * P + e % N];
    a.dx[o] = v.x;
    if (two) a.dx[o + 1] = v.y;
  }
}
