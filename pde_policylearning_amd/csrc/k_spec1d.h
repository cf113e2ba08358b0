// One-dimensional spectral convolution  y = irfft(pad(W . rfft(a)[:M]), n = N) (+ bias)  on (B, C, N) tensors, a = gelu(u) or x.
//
// In 1-D the "row" of the 2-D / 3-D kernels is the whole sample (up to 8192 points) and there is one row per (sample, channel),
// so the only parallelism is ALONG the row: the truncated DFT is a GEMM against the plan's twiddle tables, cut into slabs of
// S1_TILE points.  Three launches per direction:
//   k_s1_ana   grid (N / S1_TILE, B)   slab (C x S1_TILE) of the input through LDS as whole lines (GELU while staging), times the
//                                      (S1_TILE x 2M) table slab on the fp32 matrix cores -> partial spectrum part[b][tile][2M][C];
//                                      the gradient direction also leaves the per-slab channel sums of dy for dbias
//   k_s1_mix_*                         partials summed in tile order, scale, per-mode channel contraction (and dW, dbias)
//   k_s1_syn   grid (N / S1_TILE, B)   y slab = (C x 2M) . (2M x S1_TILE) + bias on the fp32 matrix cores, 128-byte lines out
// Arithmetic: exact fp32 everywhere (v_mfma_f32_16x16x4_f32 / v_mfma_f32_32x32x2_f32 are k-ordered fmaf chains, the mix stage is
// scalar fmaf); fno_set_gemm_mode does NOT change 1-D results.  No atomics: every sum has a fixed order, results are bitwise
// repeatable and sample b of a batch is bit for bit its own B = 1 run for y and dx.  Workspace and xhat_save hold float data only.
// Limits (checked at plan creation): C in {32, 64}, N % 128 == 0 (a short last slab where N % 256 == 128), 128 <= N <= 8192,
// 1 <= M <= 64, M <= N / 2.
#pragma once
#include "fno_dev.h"

static constexpr int S1_TILE = 256;      // points per slab: one value for all shapes (64 KB of LDS at 64 channels)

// float4 slot of column group g (4 points) of channel row r in the staged slab: rows are 64 slots (pitch 1 KB, no padding: the
// slab is exactly 64 KB at 64 channels), the XOR spreads the 16 rows x 4 groups of one ds_read_b128 wave access over all banks
FNO_DEV int s1_slot(int r, int g) { return r * (S1_TILE / 4) + (g ^ (2 * (r & 7))); }

// Analysis.  x (B, C, N); tab: 16 * ceil(2M / 16) rows of N floats (row 2k cos, 2k + 1 -sin; rows past 2M are zero);
// part (B, tiles, J = 2M, C).  dbpart (nullable): (B, tiles, C) slab sums of x.  npts: points of the LAST slab (128 or 256).
template <int C>
__global__ __launch_bounds__(256) void k_s1_ana(const float* __restrict__ x, const float* __restrict__ tab,
                                                float* __restrict__ part, float* __restrict__ dbpart, int N, int J, int act) {
  extern __shared__ float4 s1_lds[];
  const int t = blockIdx.x, b = blockIdx.y, T = gridDim.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = t * S1_TILE;
  const int npts = min(S1_TILE, N - n0);      // 256, or 128 on the last slab of an N that is an odd multiple of 128
  const float* xs = x + (size_t)b * C * N + n0;
  for (int r = wave; r < C; r += 4) {         // one channel row (1 KB) per wave and pass
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (4 * lane < npts) v = *reinterpret_cast<const float4*>(xs + (size_t)r * N + 4 * lane);
    if (act) { v.x = gelu_f(v.x); v.y = gelu_f(v.y); v.z = gelu_f(v.z); v.w = gelu_f(v.w); }
    s1_lds[s1_slot(r, lane)] = v;
    if (dbpart) {                             // fixed butterfly: every lane ends with the same sum
      float s = (v.x + v.y) + (v.z + v.w);
      for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
      if (lane == 0) dbpart[((size_t)b * T + t) * C + r] = s;
    }
  }
  __syncthreads();
  // output tiles of 16 bins x 16 channels: tile q = wave + 4 a  ->  channel tile q % (C / 16), bin tile q / (C / 16)
  constexpr int NCT = C / 16;
  const int ntile = ((J + 15) >> 4) * NCT;    // <= 8 * 4
  const int i16 = lane & 15, kk = lane >> 4;
  f32x4 acc[8];
#pragma unroll
  for (int a = 0; a < 8; ++a) acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* tb = tab + n0 + 4 * kk;
  for (int k0 = 0; k0 < npts; k0 += 16) {
#pragma unroll
    for (int a = 0; a < 8; ++a) {
      const int q = wave + 4 * a;
      if (q < ntile) {                        // wave-uniform
        const int ct = q % NCT, jt = q / NCT;
        // lane (i16, kk) holds points k0 + 4 kk .. + 3 of table row jt * 16 + i16 and of channel ct * 16 + i16; step s of the
        // four 16x16x4 products sums the points k0 + 4 kk' + s over kk' (a fixed permutation of the natural order)
        const float4 av = *reinterpret_cast<const float4*>(tb + (size_t)(jt * 16 + i16) * N + k0);
        const float4 bv = s1_lds[s1_slot(ct * 16 + i16, (k0 >> 2) + kk)];
        acc[a] = mfma16(av.x, bv.x, acc[a]);
        acc[a] = mfma16(av.y, bv.y, acc[a]);
        acc[a] = mfma16(av.z, bv.z, acc[a]);
        acc[a] = mfma16(av.w, bv.w, acc[a]);
      }
    }
  }
  float* po = part + ((size_t)b * T + t) * J * C;
#pragma unroll
  for (int a = 0; a < 8; ++a) {
    const int q = wave + 4 * a;
    if (q < ntile) {
      const int ct = q % NCT, jt = q / NCT;
#pragma unroll
      for (int r = 0; r < 4; ++r) {           // D: column (channel) = lane & 15, row (bin) = (lane >> 4) * 4 + r
        const int j = jt * 16 + kk * 4 + r;
        if (j < J) po[(size_t)j * C + ct * 16 + i16] = acc[a][r];
      }
    }
  }
}

// complex weight element (i, o, k) of either the caller's corner tensor (Cin, Cout, wl) or the packed copy [M][Cin][Cout] the
// forward leaves behind the saved spectrum: strides in float2 units
struct S1Weights { const float2* p; int si, so, sk; };

// Forward mix, grid (M, ceil(B / 16)).  part (B, T, 2M, Cin) -> X = scale * sum_t (tile order) -> xhat (B, M, Cin) complex;
// Y[b, o] = sum_i X[b, i] W[i, o, k] (i ascending) -> yhat (B, 2M, Cout).  wpack (nullable): [M][Cin][Cout] copy of the weights.
__global__ __launch_bounds__(256) void k_s1_mix_fwd(const float* __restrict__ part, S1Weights w, float2* __restrict__ xhat,
                                                    float2* __restrict__ wpack, float* __restrict__ yhat, int B, int T, int M,
                                                    int Cin, int Cout, float scale) {
  extern __shared__ float4 s1_lds[];
  float2* Ws = reinterpret_cast<float2*>(s1_lds);      // [Cin][Cout + 1]
  float2* Xs = Ws + Cin * (Cout + 1);                   // [16][Cin]
  const int k = blockIdx.x, b0 = blockIdx.y * 16, nb = min(16, B - b0), J = 2 * M;
  for (int e = threadIdx.x; e < Cin * Cout; e += 256) {
    const int i = e / Cout, o = e % Cout;
    const float2 v = w.p[(size_t)i * w.si + (size_t)o * w.so + (size_t)k * w.sk];
    Ws[i * (Cout + 1) + o] = v;
    if (wpack && blockIdx.y == 0) wpack[(size_t)k * Cin * Cout + e] = v;
  }
  for (int e = threadIdx.x; e < nb * Cin; e += 256) {
    const int bb = e / Cin, i = e % Cin;
    const float* p = part + ((size_t)(b0 + bb) * T * J + 2 * k) * Cin + i;
    float re = 0.f, im = 0.f;
    for (int t = 0; t < T; ++t) { re += p[(size_t)t * J * Cin]; im += p[(size_t)t * J * Cin + Cin]; }
    const float2 X = make_float2(scale * re, scale * im);
    Xs[e] = X;
    if (xhat) xhat[((size_t)(b0 + bb) * M + k) * Cin + i] = X;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < nb * Cout; e += 256) {
    const int bb = e / Cout, o = e % Cout;
    float re = 0.f, im = 0.f;
    for (int i = 0; i < Cin; ++i) {
      const float2 X = Xs[bb * Cin + i], Wv = Ws[i * (Cout + 1) + o];
      re = fmaf(X.x, Wv.x, re); re = fmaf(-X.y, Wv.y, re);
      im = fmaf(X.x, Wv.y, im); im = fmaf(X.y, Wv.x, im);
    }
    float* yo = yhat + ((size_t)(b0 + bb) * J + 2 * k) * Cout + o;
    yo[0] = re;
    yo[Cout] = im;
  }
}

// Backward mix, grid (M): one workgroup per kept mode walks the batch in index order, 8 samples at a time.
//   G = scale * sum_t part (B, T, 2M, Cout)                     the gradient spectrum
//   dw[i, o, k] = sum_b conj(X[b, i, k]) G[b, o, k]             (dw nullable; written at stride wl, the dead bins untouched)
//   GX[b, i] = sum_o G[b, o] conj(W[i, o, k]) -> gxhat (B, 2M, Cin)   (gxhat nullable)
//   dbias[o] = sum_b sum_t dbpart[b][t][o]                      (dbias nullable; workgroup 0)
__global__ __launch_bounds__(256) void k_s1_mix_bwd(const float* __restrict__ part, const float2* __restrict__ xhat, S1Weights w,
                                                    float2* __restrict__ dw, int wl, float* __restrict__ gxhat,
                                                    const float* __restrict__ dbpart, float* __restrict__ dbias, int B, int T,
                                                    int M, int Cin, int Cout, float scale) {
  extern __shared__ float4 s1_lds[];
  float2* Ws = reinterpret_cast<float2*>(s1_lds);      // [Cin][Cout + 1]
  float2* Gs = Ws + Cin * (Cout + 1);                   // [8][Cout]
  float2* Xs = Gs + 8 * Cout;                           // [8][Cin]
  const int k = blockIdx.x, J = 2 * M;
  const int npair = Cin * Cout / 256;                   // (i, o) pairs per thread: 4, 8 or 16
  if (gxhat)
    for (int e = threadIdx.x; e < Cin * Cout; e += 256) {
      const int i = e / Cout, o = e % Cout;
      Ws[i * (Cout + 1) + o] = w.p[(size_t)i * w.si + (size_t)o * w.so + (size_t)k * w.sk];
    }
  float2 acc[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = make_float2(0.f, 0.f);
  for (int b0 = 0; b0 < B; b0 += 8) {
    const int nb = min(8, B - b0);
    __syncthreads();                                    // the previous chunk's readers are done (and Ws is complete)
    for (int e = threadIdx.x; e < nb * Cout; e += 256) {
      const int bb = e / Cout, o = e % Cout;
      const float* p = part + ((size_t)(b0 + bb) * T * J + 2 * k) * Cout + o;
      float re = 0.f, im = 0.f;
      for (int t = 0; t < T; ++t) { re += p[(size_t)t * J * Cout]; im += p[(size_t)t * J * Cout + Cout]; }
      Gs[e] = make_float2(scale * re, scale * im);
    }
    if (dw)
      for (int e = threadIdx.x; e < nb * Cin; e += 256) {
        const int bb = e / Cin, i = e % Cin;
        Xs[e] = xhat[((size_t)(b0 + bb) * M + k) * Cin + i];
      }
    __syncthreads();
    if (dw) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        if (q < npair) {
          const int e = threadIdx.x + 256 * q, i = e / Cout, o = e % Cout;
          for (int bb = 0; bb < nb; ++bb) {
            const float2 X = Xs[bb * Cin + i], G = Gs[bb * Cout + o];
            acc[q].x = fmaf(X.x, G.x, acc[q].x); acc[q].x = fmaf(X.y, G.y, acc[q].x);
            acc[q].y = fmaf(X.x, G.y, acc[q].y); acc[q].y = fmaf(-X.y, G.x, acc[q].y);
          }
        }
      }
    }
    if (gxhat)
      for (int e = threadIdx.x; e < nb * Cin; e += 256) {
        const int bb = e / Cin, i = e % Cin;
        float re = 0.f, im = 0.f;
        for (int o = 0; o < Cout; ++o) {
          const float2 G = Gs[bb * Cout + o], Wv = Ws[i * (Cout + 1) + o];
          re = fmaf(G.x, Wv.x, re); re = fmaf(G.y, Wv.y, re);
          im = fmaf(G.y, Wv.x, im); im = fmaf(-G.x, Wv.y, im);
        }
        float* go = gxhat + ((size_t)(b0 + bb) * J + 2 * k) * Cin + i;
        go[0] = re;
        go[Cin] = im;
      }
  }
  if (dw) {
#pragma unroll
    for (int q = 0; q < 16; ++q)
      if (q < npair) {
        const int e = threadIdx.x + 256 * q, i = e / Cout, o = e % Cout;
        dw[((size_t)i * Cout + o) * wl + k] = acc[q];
      }
  }
  if (dbias && k == 0 && threadIdx.x < Cout) {
    float s = 0.f;
    for (int r = 0; r < B * T; ++r) s += dbpart[(size_t)r * Cout + threadIdx.x];
    dbias[threadIdx.x] = s;
  }
}

// Synthesis.  yhat (B, J = 2M, C) -> y (B, C, N) = sum_j yhat[b][j][c] * tab[j][n] + bias[c]; tab: J rows of N floats.
// Wave w owns columns [64 w, 64 w + 64) of the slab: C / 32 x 2 tiles of 32 x 32, natural bin order (two bins per product).
template <int C>
__global__ __launch_bounds__(256) void k_s1_syn(const float* __restrict__ yhat, const float* __restrict__ tab,
                                                const float* __restrict__ bias, float* __restrict__ y, int N, int J) {
  extern __shared__ float4 s1_lds[];
  float* ys = reinterpret_cast<float*>(s1_lds);         // [J][C]
  const int t = blockIdx.x, b = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float4* src = reinterpret_cast<const float4*>(yhat + (size_t)b * J * C);
  for (int e = threadIdx.x; e < J * C / 4; e += 256) s1_lds[e] = src[e];
  __syncthreads();
  const int n0 = t * S1_TILE + 64 * wave;
  if (n0 >= N) return;                                  // the short last slab (128 points): waves 2 and 3 have no columns
  constexpr int NCT = C / 32;
  const int l32 = lane & 31, h = lane >> 5;
  f32x16 acc[NCT][2];
#pragma unroll
  for (int c = 0; c < NCT; ++c)
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[c][s][r] = 0.f;
  const float* tb = tab + n0 + l32;
  for (int j = 0; j < J; j += 2) {                      // J is even: row j + h exists
    const float* tr = tb + (size_t)(j + h) * N;
    const float b0 = tr[0], b1 = tr[32];
#pragma unroll
    for (int c = 0; c < NCT; ++c) {
      const float a = ys[(j + h) * C + c * 32 + l32];
      acc[c][0] = mfma32(a, b0, acc[c][0]);
      acc[c][1] = mfma32(a, b1, acc[c][1]);
    }
  }
#pragma unroll
  for (int c = 0; c < NCT; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) {                      // D: column (point) = lane & 31, row (channel) = (r & 3) + 8 (r >> 2) + 4 h
      const int o = c * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      const float bo = bias ? bias[o] : 0.f;
      float* yo = y + ((size_t)b * C + o) * N + n0 + l32;
      yo[0] = acc[c][0][r] + bo;
      yo[32] = acc[c][1][r] + bo;
    }
}
