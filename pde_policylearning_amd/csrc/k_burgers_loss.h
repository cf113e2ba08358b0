// Burgers residual loss of the PINO models: FDM_Burgers + PINO_loss (libs/pino_utils/losses.py:200-243), forward and backward.
//   u (B, nt, nx), x contiguous and periodic, domain length 1, dt = 1 / (nt - 1)
//   Du[b, j] = (u[b, j+1] - u[b, j-1]) / (2 dt) + ux[b, j] u[b, j] - visc uxx[b, j]   on the interior rows j = 1 .. nt-2
//   loss_f = mean Du^2,  loss_u = mean (u[:, 0] - u0)^2
// ux = D1 u and uxx = D2 u are the real circulant operators of irfft(m(k) fft(u)[: nx/2 + 1]): m1 = 2 pi i k WITHOUT the
// Nyquist bin (its coefficient is purely imaginary there and irfft drops it), m2 = -(2 pi k)^2 WITH it (-(pi nx)^2).
//
// One workgroup owns BURG_TJ consecutive time rows of one sample and one halo row on each side, all in LDS.  Both operators
// are real and linear, so two real rows a, b travel as ONE complex line a + i b: D(a + i b) = D a + i D b, which costs one
// forward transform and one inverse per operator for the pair - no Hermitian split, and no line ever mixes ux with the
// (pi nx)^2 times larger uxx.  Transforms are fft_lines of k_pino_loss.h (radix-2, forward natural -> bit-reversed, inverse
// back), the multipliers are applied at the bit-reversed positions, lines are padded to N + 1 float2 like the NS planes.
//   forward : lines [0, TJ/2) hold the pairs; after the forward transform lines [TJ/2, TJ) take m1 Z and [0, TJ/2) m2 Z; one
//             inverse over all TJ lines.  Du and ux go to the workspace, sum Du^2 as one float64 partial per workgroup.
//   backward: r = g_f 2 Du / (B (nt-2) nx) on the interior rows, 0 on rows 0 and nt-1;
//             du = r ux - D1(r u) - visc D2 r + (r[j-1] - r[j+1]) / (2 dt) + [j = 0] g_u 2 (u - u0) / (B nx).
//             Lines [0, TJ/2) hold the pairs of r u, [TJ/2, TJ) the pairs of r: one forward over TJ lines, the combination
//             -m1 Z1 - visc m2 Z2 in [0, TJ/2), one inverse.  The shift reads r of the rows above and below the tile from
//             the stored Du (they belong to other workgroups), which is why the forward stores it.
// The means are float64 sums in a fixed order (lane -> wave -> workgroup partial -> k_burgers_finish): bitwise repeatable,
// no atomics.
#pragma once
#include "k_pino_loss.h"

constexpr int BURG_TJ = 8;       // rows per workgroup: B 20 x nt 101 gives 20 x 13 = 260 workgroups for 256 CUs
constexpr int BURG_NT = 256;     // threads (4 waves)

struct BurgersArgs {
  const float* u;        // (B, nt, nx)
  const float* u0;       // (B, nx)
  float* Du;             // workspace: (B, nt-2, nx)
  float* ux;             // workspace: (B, nt-2, nx)
  double* part_f;        // (B * tiles) sums of Du^2 (forward tiling)
  double* part_u;        // (B) sums of (u[:, 0] - u0)^2
  const float* g_u;      // backward: device scalars or null (= 1)
  const float* g_f;
  float* du;             // backward: (B, nt, nx)
  int B, nt, tiles;      // tiles: of the launching direction
  float visc, inv2dt;
  float scale_f, scale_u;   // 2 / (B (nt-2) nx), 2 / (B nx)
};

// 2 pi k and (2 pi k)^2 of the bin at bit-reversed position q, rounded once from float64; k(bin) = bin < N/2 ? bin : bin - N.
// a1 is zero in the Nyquist bin, a2 is not.
template <int N>
FNO_DEV void burgers_mult(int q, float& a1, float& a2) {
  const int bin = brev_n<N>(q);
  const double k = (double)(bin < N / 2 ? bin : bin - N);
  const double a = 6.283185307179586476925 * k;
  a1 = bin == N / 2 ? 0.f : (float)a;
  a2 = (float)(a * a);
}

// sum over the workgroup in a fixed order; the result is valid in thread 0
FNO_DEV double burgers_block_sum(double v, double* red, int tid) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

template <int N>
__global__ void __launch_bounds__(BURG_NT) k_burgers_fwd(BurgersArgs a) {
  constexpr int P = N + 1, TJ = BURG_TJ, NT = BURG_NT, NWV = NT / 64, H = TJ / 2;
  __shared__ __attribute__((aligned(16))) float2 G[TJ * P];
  __shared__ float2 tw[N / 2];
  __shared__ float Us[(TJ + 2) * N];
  __shared__ double red[NWV];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
  const int j0 = 1 + tile * TJ;                     // first interior row of the tile; Us row r is time row j0 - 1 + r
  const float* ub = a.u + (size_t)b * a.nt * N;
  for (int k = tid; k < N / 2; k += NT) {
    float sn, cs;
    sincospif(-2.0f * (float)k / (float)N, &sn, &cs);
    tw[k] = make_float2(cs, sn);
  }
  for (int e = tid; e < (TJ + 2) * N; e += NT) {
    const int j = j0 - 1 + e / N;
    Us[e] = j < a.nt ? ub[(size_t)j * N + e % N] : 0.f;
  }
  __syncthreads();
  for (int e = tid; e < H * N; e += NT) {
    const int p = e / N, x = e % N;
    // a row past the last interior one travels as zeros (its partner's transform does not see it)
    const float va = j0 + 2 * p <= a.nt - 2 ? Us[(1 + 2 * p) * N + x] : 0.f;
    const float vb = j0 + 2 * p + 1 <= a.nt - 2 ? Us[(2 + 2 * p) * N + x] : 0.f;
    G[p * P + x] = make_float2(va, vb);
  }
  __syncthreads();
  fft_lines<N, false, NWV, H>(G, P, 1, tw, wave, lane);
  __syncthreads();
  for (int e = tid; e < H * N; e += NT) {
    const int p = e / N, q = e % N;
    float a1, a2;
    burgers_mult<N>(q, a1, a2);
    const float2 z = G[p * P + q];
    G[(H + p) * P + q] = make_float2(-a1 * z.y, a1 * z.x);      // i 2 pi k Z
    G[p * P + q] = make_float2(-a2 * z.x, -a2 * z.y);           // -(2 pi k)^2 Z
  }
  __syncthreads();
  fft_lines<N, true, NWV, TJ>(G, P, 1, tw, wave, lane);
  __syncthreads();
  const float inv_n = 1.0f / (float)N;
  double ss = 0.0;
  for (int e = tid; e < TJ * N; e += NT) {
    const int r = e / N, x = e % N, j = j0 + r;
    if (j > a.nt - 2) break;                                     // (e grows with r: every later item is past the end too)
    const float2 d1 = G[(H + (r >> 1)) * P + x], d2 = G[(r >> 1) * P + x];
    const float ux = ((r & 1) ? d1.y : d1.x) * inv_n, uxx = ((r & 1) ? d2.y : d2.x) * inv_n;
    const float ut = (Us[(r + 2) * N + x] - Us[r * N + x]) * a.inv2dt;
    const float du = ut + (ux * Us[(r + 1) * N + x] - a.visc * uxx);
    const size_t o = ((size_t)b * (a.nt - 2) + (j - 1)) * N + x;
    a.Du[o] = du;
    a.ux[o] = ux;
    ss += (double)du * (double)du;
  }
  ss = burgers_block_sum(ss, red, tid);
  if (tid == 0) a.part_f[blockIdx.x] = ss;
  if (tile == 0) {                                               // Us row 0 is time row 0 here
    __syncthreads();
    double su = 0.0;
    for (int x = tid; x < N; x += NT) {
      const float d = Us[x] - a.u0[(size_t)b * N + x];
      su += (double)d * (double)d;
    }
    su = burgers_block_sum(su, red, tid);
    if (tid == 0) a.part_u[b] = su;
  }
}

// one workgroup: both means from the partials, in a fixed order
__global__ void __launch_bounds__(256) k_burgers_finish(const double* __restrict__ part_f, int nf, const double* __restrict__ part_u,
                                                        int nu, double inv_cnt_f, double inv_cnt_u, float* __restrict__ loss_u,
                                                        float* __restrict__ loss_f) {
  __shared__ double sh[2][256];
  double sf = 0.0, su = 0.0;
  for (int k = threadIdx.x; k < nf; k += 256) sf += part_f[k];
  for (int k = threadIdx.x; k < nu; k += 256) su += part_u[k];
  sh[0][threadIdx.x] = sf; sh[1][threadIdx.x] = su;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) { sh[0][threadIdx.x] += sh[0][threadIdx.x + off]; sh[1][threadIdx.x] += sh[1][threadIdx.x + off]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    loss_f[0] = (float)(sh[0][0] * inv_cnt_f);
    loss_u[0] = (float)(sh[1][0] * inv_cnt_u);
  }
}

// du of BURG_TJ consecutive rows j0 = tile * TJ .. (all nt rows are tiled: rows 0 and nt-1 carry r = 0)
template <int N>
__global__ void __launch_bounds__(BURG_NT) k_burgers_bwd(BurgersArgs a) {
  constexpr int P = N + 1, TJ = BURG_TJ, NT = BURG_NT, NWV = NT / 64, H = TJ / 2;
  __shared__ __attribute__((aligned(16))) float2 G[TJ * P];
  __shared__ float2 tw[N / 2];
  __shared__ float Rs[(TJ + 2) * N];                 // r of time rows j0 - 1 .. j0 + TJ
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
  const int j0 = tile * TJ;
  const float* ub = a.u + (size_t)b * a.nt * N;
  const size_t wb = (size_t)b * (a.nt - 2) * N;      // the sample's interior rows in the workspace: row j at (j - 1) * N
  for (int k = tid; k < N / 2; k += NT) {
    float sn, cs;
    sincospif(-2.0f * (float)k / (float)N, &sn, &cs);
    tw[k] = make_float2(cs, sn);
  }
  const float sf = a.scale_f * (a.g_f ? a.g_f[0] : 1.0f);
  for (int e = tid; e < (TJ + 2) * N; e += NT) {
    const int j = j0 - 1 + e / N;
    Rs[e] = (j >= 1 && j <= a.nt - 2) ? sf * a.Du[wb + (size_t)(j - 1) * N + e % N] : 0.f;
  }
  __syncthreads();
  for (int e = tid; e < H * N; e += NT) {
    const int p = e / N, x = e % N, ja = j0 + 2 * p, jb = ja + 1;
    const float ra = Rs[(1 + 2 * p) * N + x], rb = Rs[(2 + 2 * p) * N + x];
    const float ua = ja < a.nt ? ub[(size_t)ja * N + x] : 0.f, uc = jb < a.nt ? ub[(size_t)jb * N + x] : 0.f;
    G[p * P + x] = make_float2(ra * ua, rb * uc);
    G[(H + p) * P + x] = make_float2(ra, rb);
  }
  __syncthreads();
  fft_lines<N, false, NWV, TJ>(G, P, 1, tw, wave, lane);
  __syncthreads();
  for (int e = tid; e < H * N; e += NT) {
    const int p = e / N, q = e % N;
    float a1, a2;
    burgers_mult<N>(q, a1, a2);
    const float2 z1 = G[p * P + q], z2 = G[(H + p) * P + q];
    const float va2 = a.visc * a2;
    // -D1(r u) - visc D2 r:  -i 2 pi k Z1 + visc (2 pi k)^2 Z2
    G[p * P + q] = make_float2(fmaf(a1, z1.y, va2 * z2.x), fmaf(-a1, z1.x, va2 * z2.y));
  }
  __syncthreads();
  fft_lines<N, true, NWV, H>(G, P, 1, tw, wave, lane);
  __syncthreads();
  const float inv_n = 1.0f / (float)N;
  const float su = a.scale_u * (a.g_u ? a.g_u[0] : 1.0f);
  for (int e = tid; e < TJ * N; e += NT) {
    const int r = e / N, x = e % N, j = j0 + r;
    if (j >= a.nt) break;
    const float2 s = G[(r >> 1) * P + x];
    float v = (Rs[r * N + x] - Rs[(r + 2) * N + x]) * a.inv2dt;
    // rows 0 and nt-1 carry r = 0: their spectral part is exactly zero, and what the line holds there is the rounding of the
    // partner row's transform (up to visc (pi nx)^2 eps |r|: more than the whole shift term on a white field)
    if (j >= 1 && j <= a.nt - 2) v += fmaf(Rs[(r + 1) * N + x], a.ux[wb + (size_t)(j - 1) * N + x], ((r & 1) ? s.y : s.x) * inv_n);
    if (j == 0) v = fmaf(su, ub[x] - a.u0[(size_t)b * N + x], v);
    a.du[((size_t)b * a.nt + j) * N + x] = v;
  }
}
