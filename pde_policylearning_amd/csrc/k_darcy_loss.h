// Darcy residual loss of the PINO models: FDM_Darcy + darcy_loss (libs/pino_utils/losses.py:6-65) with the mollifier and the
// relative-L2 data term of the training loop (train_2d.py:58-82) folded in, forward and backward.
//   out, a, y (B, S, S), first grid index x, h = 1 / (S - 1);  pred = out * mol  (mol (S, S) or absent: pred = out)
//   Du[b, p, q] = -( a[p+1,q] (pred[p+2,q] - pred[p,q]) - a[p-1,q] (pred[p,q] - pred[p-2,q])
//                  + a[p,q+1] (pred[p,q+2] - pred[p,q]) - a[p,q-1] (pred[p,q] - pred[p,q-2]) ) / (4 h^2),   p, q = 2 .. S-3
//   loss_f = mean_b ||Du_b - 1||_2 / (S - 4),   loss_data = mean_b ||pred_b - y_b||_2 / ||y_b||_2
// which is FDM_Darcy's sliced form (a ux, a uy differenced once more) written per cell.
//
// A sample's residual cells [2, S-3]^2 are cut into DARCY_T x DARCY_T tiles; one workgroup owns one tile of one sample and
// keeps pred with a two-cell halo and a with a one-cell halo in LDS.  For the sums over ALL S x S cells (the data term) and
// for dout every cell needs one owner: the tiles on the rim of the tiling also own the two-cell ring outside the residual
// cells (`darcy_own`), which their halo already holds.
//   forward : Du to the workspace as (B, S-4, S-4); sums of (Du-1)^2, (pred-y)^2, y^2 as three float64 partials per workgroup.
//   finish  : per-sample norms (float64, kept in the workspace) from the partials, one wave per sample, then the two means.
//   backward: r = g_f (Du - 1) / (B (S-4) ||Du_b - 1||) on the residual cells, 0 elsewhere (a sample whose norm is exactly
//             zero gives r = 0 where the reference's 0 / 0 gives NaN), read from the stored Du with a four-cell apron;
//             dpred[m,n] = -( a[m-1,n] r[m-2,n] + a[m+1,n] r[m+2,n] - (a[m+1,n] + a[m-1,n]) r[m,n]
//                           + a[m,n-1] r[m,n-2] + a[m,n+1] r[m,n+2] - (a[m,n+1] + a[m,n-1]) r[m,n] ) / (4 h^2)
//                         + g_data (pred - y)[m,n] / (B ||pred_b - y_b|| ||y_b||),   dout = mol * dpred.
//             Every cell of dout is written once, by its owner.
// Sums run lane -> wave -> workgroup partial -> k_darcy_finish in a fixed order: bitwise repeatable, no atomics, and sample b
// of a batch sees exactly the operations of its B = 1 run.
#pragma once
#include "k_burgers_loss.h"

constexpr int DARCY_T = 16;                  // tile extent in residual cells: S 61 gives 4 x 4 tiles, B 20 -> 320 workgroups
constexpr int DARCY_NT = DARCY_T * DARCY_T;  // threads: one per residual cell of the tile (4 waves)
constexpr int DARCY_SMAX = 4096;             // largest S taken (421 is the data's full grid)
static_assert(DARCY_NT == 256, "burgers_block_sum adds four waves");

struct DarcyArgs {
  const float* out;      // (B, S, S)
  const float* mol;      // (S, S) or null
  const float* a;        // (B, S, S)
  const float* y;        // (B, S, S) or null
  float* Du;             // workspace: (B, S-4, S-4)
  double* part;          // workspace: (B * tiles * tiles, 3) sums of (Du-1)^2, (pred-y)^2, y^2
  double* norms;         // workspace: (B, 3) their per-sample square roots
  const float* g_data;   // backward: device scalars or null (= 1)
  const float* g_f;
  float* dout;           // backward: (B, S, S)
  int B, S, tiles;       // tiles per direction
  float inv4h2;          // (S - 1)^2 / 4
};

// the cells [lo, hi) of one direction that tile t owns: its DARCY_T residual cells, and the two-cell ring on the rim tiles
FNO_DEV void darcy_own(int t, int tiles, int S, int& lo, int& hi) {
  lo = t == 0 ? 0 : 2 + t * DARCY_T;
  hi = t == tiles - 1 ? S : 2 + (t + 1) * DARCY_T;
}

__global__ void __launch_bounds__(DARCY_NT) k_darcy_fwd(DarcyArgs a) {
  constexpr int T = DARCY_T, NT = DARCY_NT, PW = T + 4, AW = T + 2;
  __shared__ float Ps[PW][PW + 1];                  // pred of cells (m0 - 2 + i, n0 - 2 + j); 0 past the grid
  __shared__ float As[AW][AW + 1];                  // a of cells (m0 - 1 + i, n0 - 1 + j)
  __shared__ double red[NT / 64];
  const int tid = threadIdx.x, S = a.S;
  const int per = a.tiles * a.tiles, b = blockIdx.x / per, tile = blockIdx.x % per;
  const int tx = tile / a.tiles, ty = tile % a.tiles;
  const int m0 = 2 + tx * T, n0 = 2 + ty * T;       // first residual cell of the tile
  const size_t sb = (size_t)b * S * S;
  for (int e = tid; e < PW * PW; e += NT) {
    const int i = e / PW, j = e % PW, m = m0 - 2 + i, n = n0 - 2 + j;
    float v = 0.f;
    if (m < S && n < S) {
      v = a.out[sb + (size_t)m * S + n];
      if (a.mol) v *= a.mol[(size_t)m * S + n];
    }
    Ps[i][j] = v;
  }
  for (int e = tid; e < AW * AW; e += NT) {
    const int i = e / AW, j = e % AW, m = m0 - 1 + i, n = n0 - 1 + j;
    As[i][j] = (m < S && n < S) ? a.a[sb + (size_t)m * S + n] : 0.f;
  }
  __syncthreads();
  double sf = 0.0, sd = 0.0, sy = 0.0;
  {
    const int i = tid / T, j = tid % T, p = m0 + i, q = n0 + j;
    if (p <= S - 3 && q <= S - 3) {
      const float c = Ps[i + 2][j + 2];
      const float fx = As[i + 2][j + 1] * (Ps[i + 4][j + 2] - c) - As[i][j + 1] * (c - Ps[i][j + 2]);
      const float fy = As[i + 1][j + 2] * (Ps[i + 2][j + 4] - c) - As[i + 1][j] * (c - Ps[i + 2][j]);
      const float du = -(fx + fy) * a.inv4h2;
      a.Du[((size_t)b * (S - 4) + (p - 2)) * (S - 4) + (q - 2)] = du;
      const double d = (double)du - 1.0;
      sf = d * d;
    }
  }
  if (a.y) {
    int mlo, mhi, nlo, nhi;
    darcy_own(tx, a.tiles, S, mlo, mhi);
    darcy_own(ty, a.tiles, S, nlo, nhi);
    const int ow = nhi - nlo, cnt = (mhi - mlo) * ow;
    for (int e = tid; e < cnt; e += NT) {
      const int m = mlo + e / ow, n = nlo + e % ow;
      const float yv = a.y[sb + (size_t)m * S + n];
      const double d = (double)(Ps[m - (m0 - 2)][n - (n0 - 2)] - yv);
      sd += d * d;
      sy += (double)yv * (double)yv;
    }
  }
  sf = burgers_block_sum(sf, red, tid);
  __syncthreads();
  sd = burgers_block_sum(sd, red, tid);
  __syncthreads();
  sy = burgers_block_sum(sy, red, tid);
  if (tid == 0) {
    double* o = a.part + (size_t)blockIdx.x * 3;
    o[0] = sf; o[1] = sd; o[2] = sy;
  }
}

// one workgroup: per-sample norms from the partials, then both means, all in a fixed order
__global__ void __launch_bounds__(256) k_darcy_finish(const double* __restrict__ part, int B, int per, int S,
                                                      double* __restrict__ norms, float* __restrict__ loss_data,
                                                      float* __restrict__ loss_f) {
  // one wave per sample (b = wave, wave + 4, ..): lane l adds tiles l, l + 64, .., then the xor butterfly, whose sum is the
  // same in every lane and depends on the sample's own partials alone
  __shared__ double sh[2][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double af = 0.0, ad = 0.0;
  for (int b = wave; b < B; b += 4) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    const double* p = part + (size_t)b * per * 3;
    for (int t = lane; t < per; t += 64) { s0 += p[3 * t]; s1 += p[3 * t + 1]; s2 += p[3 * t + 2]; }
    for (int off = 32; off > 0; off >>= 1) {
      s0 += __shfl_xor(s0, off, 64); s1 += __shfl_xor(s1, off, 64); s2 += __shfl_xor(s2, off, 64);
    }
    const double nf = sqrt(s0), nd = sqrt(s1), ny = sqrt(s2);
    if (lane == 0) { norms[3 * b] = nf; norms[3 * b + 1] = nd; norms[3 * b + 2] = ny; }
    af += nf / (double)(S - 4);
    if (loss_data) ad += nd / ny;
  }
  if (lane == 0) { sh[0][wave] = af; sh[1][wave] = ad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    loss_f[0] = (float)(((sh[0][0] + sh[0][1]) + (sh[0][2] + sh[0][3])) / (double)B);
    if (loss_data) loss_data[0] = (float)(((sh[1][0] + sh[1][1]) + (sh[1][2] + sh[1][3])) / (double)B);
  }
}

__global__ void __launch_bounds__(DARCY_NT) k_darcy_bwd(DarcyArgs a) {
  constexpr int T = DARCY_T, NT = DARCY_NT, RW = T + 8, AW = T + 6;
  __shared__ float Rs[RW][RW + 1];                  // r of cells (m0 - 4 + i, n0 - 4 + j); 0 off the residual cells
  __shared__ float As[AW][AW + 1];                  // a of cells (m0 - 3 + i, n0 - 3 + j); 0 off the grid
  const int tid = threadIdx.x, S = a.S;
  const int per = a.tiles * a.tiles, b = blockIdx.x / per, tile = blockIdx.x % per;
  const int tx = tile / a.tiles, ty = tile % a.tiles;
  const int m0 = 2 + tx * T, n0 = 2 + ty * T;
  const size_t sb = (size_t)b * S * S, wb = (size_t)b * (S - 4) * (S - 4);
  const double nf = a.norms[3 * b], nd = a.norms[3 * b + 1], ny = a.norms[3 * b + 2];
  const float gf = a.g_f ? a.g_f[0] : 1.0f, gd = a.g_data ? a.g_data[0] : 1.0f;
  const float cf = nf > 0.0 ? gf * (float)(1.0 / ((double)a.B * (double)(S - 4) * nf)) : 0.f;
  // the data term as k_lploss_finish scales it: 0 where the difference vanishes (torch.norm's subgradient)
  const float cd = (a.y && nd > 0.0) ? gd * (float)(1.0 / ((double)a.B * nd * ny)) : 0.f;
  for (int e = tid; e < RW * RW; e += NT) {
    const int i = e / RW, j = e % RW, m = m0 - 4 + i, n = n0 - 4 + j;
    float v = 0.f;
    if (m >= 2 && m <= S - 3 && n >= 2 && n <= S - 3) v = cf * (a.Du[wb + (size_t)(m - 2) * (S - 4) + (n - 2)] - 1.0f);
    Rs[i][j] = v;
  }
  for (int e = tid; e < AW * AW; e += NT) {
    const int i = e / AW, j = e % AW, m = m0 - 3 + i, n = n0 - 3 + j;
    As[i][j] = (m >= 0 && m < S && n >= 0 && n < S) ? a.a[sb + (size_t)m * S + n] : 0.f;
  }
  __syncthreads();
  int mlo, mhi, nlo, nhi;
  darcy_own(tx, a.tiles, S, mlo, mhi);
  darcy_own(ty, a.tiles, S, nlo, nhi);
  const int ow = nhi - nlo, cnt = (mhi - mlo) * ow;
  for (int e = tid; e < cnt; e += NT) {
    const int m = mlo + e / ow, n = nlo + e % ow;
    const int ri = m - (m0 - 4), rj = n - (n0 - 4), ai = m - (m0 - 3), aj = n - (n0 - 3);      // ri, rj >= 2; ai, aj >= 1
    const float rc = Rs[ri][rj];
    const float axm = As[ai - 1][aj], axp = As[ai + 1][aj], aym = As[ai][aj - 1], ayp = As[ai][aj + 1];
    const float gx = axm * Rs[ri - 2][rj] + axp * Rs[ri + 2][rj] - (axp + axm) * rc;
    const float gy = aym * Rs[ri][rj - 2] + ayp * Rs[ri][rj + 2] - (ayp + aym) * rc;
    float v = -(gx + gy) * a.inv4h2;
    const size_t o = sb + (size_t)m * S + n;
    const float mo = a.mol ? a.mol[(size_t)m * S + n] : 1.0f;
    if (a.y) v = fmaf(cd, a.out[o] * mo - a.y[o], v);
    a.dout[o] = a.mol ? mo * v : v;
  }
}
