// Channel MLP of an FNO block built with use_mlp=True (neuralop/models/fno_block.py:123-170, mlp.py:26-54,
// skip_connections.py:38-74), forward and backward:
//   y = [gelu]( gelu(W2 gelu(W1 u + b1) + b2) + g (.) x )
// u (B, C, PW): the Fourier part's output, x (B, C, PW): the block's input, W1 (HID, C), W2 (C, HID), g (C) the soft gate
// (null: identity skip).  The HID-wide hidden tensor and the pre-activations never leave the CU; the backward recomputes them
// from u and x.  Both GEMMs run on v_mfma_f32_32x32x2_f32 (exact fp32) in either GEMM mode: a forward pixel costs
// 4 C HID flop against 3 C floats of traffic (roofs, and what the kernels reach of them: DESIGN.md section 4u).
//
// Workgroup: 4 waves, one 128-pixel tile of one sample's plane per iteration of a persistent grid-stride loop; wave nt owns
// pixels [32 nt, +32) of the tile for every GEMM whose N dimension is pixels, so the hidden tensor goes accumulator -> LDS ->
// B operand inside the columns of one wave.  u, x, dy, y, du, dx move as 16 bytes per lane, 32 lanes per 512-byte row piece
// (whole 128-byte lines, a quarter of the requests of an accumulator-layout access: DESIGN.md section 4g); the accumulator
// layout is reached through an LDS turn.  Tile rows are PITCH = 132 floats, weight rows are padded to an odd length.
#pragma once
#include "fno_dev.h"

struct CmlpFwdArgs {
  const float *u, *x;          // (B, C, PW)
  const float *w1, *b1;        // (HID, C), (HID)
  const float *w2, *b2;        // (C, HID), (C)
  const float* g;              // (C) or null
  float* y;                    // (B, C, PW)
  int PW, tiles_per_plane, ntiles, gelu_out;
};

// dynamic LDS bytes of k_cmlp_fwd<C, HID>: the u / v tile, the t tile, W1 (rows C+1), W2 (rows HID+1), b1, b2, g
static inline size_t cmlp_fwd_lds_bytes(int C, int HID) {
  return ((size_t)(C + HID) * 132 + (size_t)HID * (C + 1) + (size_t)C * (HID + 1) + HID + 2 * C) * 4;
}
// ... of k_cmlp_bwd<C, HID>: the u tile, the v / dy' / ds / du tile, the t / dh tile and the same parameters
static inline size_t cmlp_bwd_lds_bytes(int C, int HID) {
  return ((size_t)(2 * C + HID) * 132 + (size_t)HID * (C + 1) + (size_t)C * (HID + 1) + HID + 2 * C) * 4;
}

template <int C, int HID>
FNO_DEV void cmlp_stage_params(float* w1s, float* w2s, float* b1s, float* b2s, float* gs, const float* w1, const float* b1,
                               const float* w2, const float* b2, const float* g, int tid, int nt) {
  for (int i = tid; i < HID * C; i += nt) w1s[(i / C) * (C + 1) + i % C] = w1[i];
  for (int i = tid; i < C * HID; i += nt) w2s[(i / HID) * (HID + 1) + i % HID] = w2[i];
  for (int i = tid; i < HID; i += nt) b1s[i] = b1[i];
  for (int i = tid; i < C; i += nt) { b2s[i] = b2[i]; gs[i] = g ? g[i] : 1.0f; }
}

template <int C, int HID>
__global__ void __launch_bounds__(256, 2) k_cmlp_fwd(CmlpFwdArgs a) {
  constexpr int NPX = 128, NT = 256, PITCH = NPX + 4, W1P = C + 1, W2P = HID + 1, MH = HID / 32, MC = C / 32;
  using PF = TilePrefetch<NPX, NT, C, C>;
  static_assert(PF::TOTAL % NT == 0, "whole prefetch passes");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* us = smem;                   // C x PITCH   : u, then v = gelu(W2 t + b2)
  float* ts = us + C * PITCH;         // HID x PITCH : t = gelu(W1 u + b1)
  float* w1s = ts + HID * PITCH;      // HID x W1P
  float* w2s = w1s + HID * W1P;       // C x W2P
  float* b1s = w2s + C * W2P;         // HID
  float* b2s = b1s + HID;             // C
  float* gs = b2s + C;                // C
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, half = lane >> 5;
  const int n0 = wave * 32;
  float gk_six, gk_inf;               // clamp constants of the packed GELU (fno_dev.h), in SGPRs
  gelu_consts(gk_six, gk_inf);

  cmlp_stage_params<C, HID>(w1s, w2s, b1s, b2s, gs, a.w1, a.b1, a.w2, a.b2, a.g, tid, NT);

  PF pfu, pfx;      // the next tile's u rows (in flight during this tile's GEMMs) and this tile's x rows (used by the epilogue)
  if ((int)blockIdx.x < a.ntiles) {
    const size_t off = (size_t)(blockIdx.x / a.tiles_per_plane) * C * a.PW + (size_t)(blockIdx.x % a.tiles_per_plane) * NPX;
    pfu.issue(a.u + off, a.PW, tid);
    pfx.issue(a.x + off, a.PW, tid);
  }

  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const size_t off = (size_t)(tile / a.tiles_per_plane) * C * a.PW + (size_t)(tile % a.tiles_per_plane) * NPX;
    const int nt2 = tile + gridDim.x;
    const size_t off2 = (size_t)(nt2 / a.tiles_per_plane) * C * a.PW + (size_t)(nt2 % a.tiles_per_plane) * NPX;
    pfu.commit(us, false, tid);
    __syncthreads();
    if (nt2 < a.ntiles) {
      int t_ = tid;
      asm volatile("" : "+v"(t_));      // (no hoisted per-lane 64-bit prefetch addresses: k_pw_fwd_x3)
      pfu.issue(a.u + off2, a.PW, t_);
    }
    // ---- t = gelu(W1 u + b1): accumulator -> LDS, inside this wave's 32 columns
    {
      f32x16 acc[MH];
#pragma unroll
      for (int m = 0; m < MH; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
      const float* xp = us + half * PITCH + n0 + l31;
#pragma unroll
      for (int m = 0; m < MH; ++m) {
        const float* wp = w1s + (m * 32 + l31) * W1P + half;
#pragma unroll
        for (int s = 0; s < C / 2; ++s) acc[m] = mfma32(wp[2 * s], xp[2 * s * PITCH], acc[m]);
      }
#pragma unroll
      for (int m = 0; m < MH; ++m) {      // the activation on pairs (fno_dev.h: gelu_pairs): 16 rows of this lane's pixel
        f32x2 hp[8];
#pragma unroll
        for (int r = 0; r < 16; ++r) hp[r >> 1][r & 1] = acc[m][r] + b1s[m * 32 + acc_row32(r, half)];
        gelu_pairs<8>(hp, gk_six, gk_inf);
#pragma unroll
        for (int r = 0; r < 16; ++r) ts[(m * 32 + acc_row32(r, half)) * PITCH + n0 + l31] = hp[r >> 1][r & 1];
      }
    }
    __syncthreads();
    // ---- v = gelu(W2 t + b2) -> the u tile's place (every wave is past its reads of u)
    {
      f32x16 acc[MC];
#pragma unroll
      for (int m = 0; m < MC; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
      const float* tp = ts + half * PITCH + n0 + l31;
#pragma unroll
      for (int m = 0; m < MC; ++m) {
        const float* wp = w2s + (m * 32 + l31) * W2P + half;
#pragma unroll
        for (int s = 0; s < HID / 2; ++s) acc[m] = mfma32(wp[2 * s], tp[2 * s * PITCH], acc[m]);
      }
#pragma unroll
      for (int m = 0; m < MC; ++m) {
        f32x2 hp[8];
#pragma unroll
        for (int r = 0; r < 16; ++r) hp[r >> 1][r & 1] = acc[m][r] + b2s[m * 32 + acc_row32(r, half)];
        gelu_pairs<8>(hp, gk_six, gk_inf);
#pragma unroll
        for (int r = 0; r < 16; ++r) us[(m * 32 + acc_row32(r, half)) * PITCH + n0 + l31] = hp[r >> 1][r & 1];
      }
    }
    __syncthreads();
    // ---- y = [gelu](v + g x): 16 bytes per lane, whole lines
#pragma unroll
    for (int i = 0; i < PF::ITER; ++i) {
      const int idx = tid + i * NT;
      const int c = idx / (NPX / 4), q = idx % (NPX / 4);
      const float4 v = ld4(us + c * PITCH + 4 * q);
      const float4 xv = pfx.v[i];
      const float gc = gs[c];
      float4 y = make_float4(fmaf(gc, xv.x, v.x), fmaf(gc, xv.y, v.y), fmaf(gc, xv.z, v.z), fmaf(gc, xv.w, v.w));
      if (a.gelu_out) y = gelu4(y, gk_six, gk_inf);
      st4(a.y + off + (size_t)c * a.PW + 4 * q, y);
    }
    if (nt2 < a.ntiles) {
      int t_ = tid;
      asm volatile("" : "+v"(t_));
      pfx.issue(a.x + off2, a.PW, t_);
    }
    __syncthreads();      // the epilogue's reads of the tile before the next commit
  }
}

struct CmlpBwdArgs {
  const float *u, *x, *dy;     // (B, C, PW)
  const float *w1, *b1, *w2, *b2;
  const float* g;              // (C) or null
  float* du;                   // (B, C, PW)
  float* dx;                   // (B, C, PW) or null: not wanted
  float* dw1_part;             // (gridDim * KSPLIT, HID, C)
  float* db1_part;             // (gridDim * 4, HID)
  float* dw2_part;             // (gridDim * KSPLIT, C, HID)
  float* db2_part;             // (gridDim * 4, C)
  float* dg_part;              // (gridDim, C) or null
  int PW, tiles_per_plane, ntiles, gelu_out;
};

// the weight-gradient products (K = the tile's 128 pixels) have (C/32)(HID/32) output tiles for 4 waves: with fewer tiles than
// waves the pixels are split, and every (tile, pixel part) leaves its own partial slab
template <int C, int HID>
struct CmlpBwdCfg {
  static constexpr int TILES = (C / 32) * (HID / 32);
  static constexpr int KSPLIT = 4 / TILES;
  static_assert(TILES == 1 || TILES == 2 || TILES == 4, "weight-gradient tiling");
};
static inline int cmlp_bwd_ksplit(int C, int HID) { return 4 / ((C / 32) * (HID / 32)); }

// Per tile (barriers between the steps; "own columns" = pixels [32 wave, +32)):
//   1  h = W1 u + b1 (own columns);  t = gelu(h) -> LDS, gelu'(h) stays in registers
//   2  s = W2 t + b2 (own columns);  gelu'(s) stays in registers; with gelu_out, v = gelu(s) -> LDS
//   3  whole lines: dy' = dy gelu'(v + g x) (gelu_out) or dy; dx = g dy' stored; dg += dy' x per lane; dy' -> LDS
//   4  ds = dy' gelu'(s) in place (own columns); db2 += ds
//   5  dt = W2^T ds (own columns);  dW2 += ds t^T (this wave's tile and pixel part)
//   6  dh = dt gelu'(h) -> LDS over t (own columns); db1 += dh
//   7  du = W1^T dh (own columns);  dW1 += dh u^T;  du -> LDS over ds
//   8  whole lines: du stored
// db1 / db2 are reduced over the wave's 32 columns per tile (half_reduce16), dg over lanes after the last tile; every workgroup leaves one set of partials and a
// fixed-order reduction (k_reduce_jobs) follows: no floating-point atomics, the same bits run to run.
template <int C, int HID>
__global__ void __launch_bounds__(256, 1) k_cmlp_bwd(CmlpBwdArgs a) {
  constexpr int NPX = 128, NT = 256, PITCH = NPX + 4, W1P = C + 1, W2P = HID + 1, MH = HID / 32, MC = C / 32;
  using Cfg = CmlpBwdCfg<C, HID>;
  constexpr int KSPLIT = Cfg::KSPLIT, KPX = NPX / KSPLIT;
  using PF = TilePrefetch<NPX, NT, C, C>;
  static_assert(PF::TOTAL % NT == 0 && NT % (NPX / 4) == 0, "whole prefetch passes, one channel per lane and pass");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* us = smem;                   // C x PITCH   : u
  float* bs = us + C * PITCH;         // C x PITCH   : v, dy', ds, du in turn
  float* ts = bs + C * PITCH;         // HID x PITCH : t, then dh
  float* w1s = ts + HID * PITCH;      // HID x W1P
  float* w2s = w1s + HID * W1P;       // C x W2P
  float* b1s = w2s + C * W2P;         // HID
  float* b2s = b1s + HID;             // C
  float* gs = b2s + C;                // C
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, half = lane >> 5;
  const int n0 = wave * 32;
  const int wt = wave % Cfg::TILES, kpart = wave / Cfg::TILES;      // this wave's weight-gradient tile and pixel part
  const int wmc = wt / MH, wmh = wt % MH;                           // ... its channel and hidden 32-blocks

  cmlp_stage_params<C, HID>(w1s, w2s, b1s, b2s, gs, a.w1, a.b1, a.w2, a.b2, a.g, tid, NT);

  f32x16 dw1acc, dw2acc;
  // lane accumulates the bias gradient of row  32 m + acc_row32(reduce16_id(lane), half)  of its wave's 32 columns
  float sdb1[MH], sdb2[MC], sdg[PF::ITER];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    dw1acc[r] = 0.f;
    dw2acc[r] = 0.f;
  }
#pragma unroll
  for (int m = 0; m < MH; ++m) sdb1[m] = 0.f;
#pragma unroll
  for (int m = 0; m < MC; ++m) sdb2[m] = 0.f;
#pragma unroll
  for (int i = 0; i < PF::ITER; ++i) sdg[i] = 0.f;

  PF pfu;      // the next tile's u rows, in flight during this tile
  if ((int)blockIdx.x < a.ntiles)
    pfu.issue(a.u + (size_t)(blockIdx.x / a.tiles_per_plane) * C * a.PW + (size_t)(blockIdx.x % a.tiles_per_plane) * NPX, a.PW, tid);

  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const size_t off = (size_t)(tile / a.tiles_per_plane) * C * a.PW + (size_t)(tile % a.tiles_per_plane) * NPX;
    const int nt2 = tile + gridDim.x;
    const size_t off2 = (size_t)(nt2 / a.tiles_per_plane) * C * a.PW + (size_t)(nt2 % a.tiles_per_plane) * NPX;
    pfu.commit(us, false, tid);
    __syncthreads();
    if (nt2 < a.ntiles) {
      int t_ = tid;
      asm volatile("" : "+v"(t_));      // (no hoisted per-lane 64-bit prefetch addresses: k_pw_fwd_x3)
      pfu.issue(a.u + off2, a.PW, t_);
    }
    PF pfx, pfd;      // this tile's x and dy rows: wanted in step 3, in flight during steps 1 and 2
    {
      int t_ = tid;
      asm volatile("" : "+v"(t_));
      pfx.issue(a.x + off, a.PW, t_);
      pfd.issue(a.dy + off, a.PW, t_);
    }
    // ---- 1
    float dgh[MH][16];
    {
      f32x16 acc[MH];
#pragma unroll
      for (int m = 0; m < MH; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
      const float* xp = us + half * PITCH + n0 + l31;
#pragma unroll
      for (int m = 0; m < MH; ++m) {
        const float* wp = w1s + (m * 32 + l31) * W1P + half;
#pragma unroll 8
        for (int s = 0; s < C / 2; ++s) acc[m] = mfma32(wp[2 * s], xp[2 * s * PITCH], acc[m]);
      }
#pragma unroll
      for (int m = 0; m < MH; ++m) {      // value and derivative on pairs (fno_dev.h: gelu_both_pairs)
        f32x2 hp[8], gv[8], dv[8];
#pragma unroll
        for (int r = 0; r < 16; ++r) hp[r >> 1][r & 1] = acc[m][r] + b1s[m * 32 + acc_row32(r, half)];
        gelu_both_pairs<8>(hp, gv, dv);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          ts[(m * 32 + acc_row32(r, half)) * PITCH + n0 + l31] = gv[r >> 1][r & 1];
          dgh[m][r] = dv[r >> 1][r & 1];
        }
      }
    }
    __syncthreads();
    // ---- 2
    float dgs[MC][16];
    {
      f32x16 acc[MC];
#pragma unroll
      for (int m = 0; m < MC; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
      const float* tp = ts + half * PITCH + n0 + l31;
#pragma unroll
      for (int m = 0; m < MC; ++m) {
        const float* wp = w2s + (m * 32 + l31) * W2P + half;
#pragma unroll 8
        for (int s = 0; s < HID / 2; ++s) acc[m] = mfma32(wp[2 * s], tp[2 * s * PITCH], acc[m]);
      }
#pragma unroll
      for (int m = 0; m < MC; ++m) {
        f32x2 hp[8], gv[8], dv[8];
#pragma unroll
        for (int r = 0; r < 16; ++r) hp[r >> 1][r & 1] = acc[m][r] + b2s[m * 32 + acc_row32(r, half)];
        gelu_both_pairs<8>(hp, gv, dv);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if (a.gelu_out) bs[(m * 32 + acc_row32(r, half)) * PITCH + n0 + l31] = gv[r >> 1][r & 1];
          dgs[m][r] = dv[r >> 1][r & 1];
        }
      }
    }
    __syncthreads();
    // ---- 3
#pragma unroll
    for (int i = 0; i < PF::ITER; ++i) {
      const int idx = tid + i * NT;
      const int c = idx / (NPX / 4), q = idx % (NPX / 4);
      const float4 xv = pfx.v[i];
      float4 d = pfd.v[i];
      const float gc = gs[c];
      if (a.gelu_out) {
        const float4 v = ld4(bs + c * PITCH + 4 * q);
        float4 yp = make_float4(fmaf(gc, xv.x, v.x), fmaf(gc, xv.y, v.y), fmaf(gc, xv.z, v.z), fmaf(gc, xv.w, v.w)), dd;
        gelu_both4(yp, dd);
        d.x *= dd.x; d.y *= dd.y; d.z *= dd.z; d.w *= dd.w;
      }
      sdg[i] += (d.x * xv.x + d.y * xv.y) + (d.z * xv.z + d.w * xv.w);
      if (a.dx) st4(a.dx + off + (size_t)c * a.PW + 4 * q, make_float4(gc * d.x, gc * d.y, gc * d.z, gc * d.w));
      st4(bs + c * PITCH + 4 * q, d);
    }
    __syncthreads();
    // ---- 4
#pragma unroll
    for (int m = 0; m < MC; ++m) {
      float dsv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float* p = bs + (m * 32 + acc_row32(r, half)) * PITCH + n0 + l31;
        dsv[r] = *p * dgs[m][r];
        *p = dsv[r];
      }
      sdb2[m] += half_reduce16(dsv, lane);
    }
    __syncthreads();
    // ---- 5
    f32x16 accdt[MH];
    {
#pragma unroll
      for (int m = 0; m < MH; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) accdt[m][r] = 0.f;
      const float* dp = bs + half * PITCH + n0 + l31;
#pragma unroll
      for (int m = 0; m < MH; ++m) {
        const float* wp = w2s + half * W2P + m * 32 + l31;      // A[i = hidden][k = channel] = W2[channel][hidden]
#pragma unroll 8
        for (int s = 0; s < C / 2; ++s) accdt[m] = mfma32(wp[2 * s * W2P], dp[2 * s * PITCH], accdt[m]);
      }
      const float* ga = bs + (wmc * 32 + l31) * PITCH + kpart * KPX + 4 * half;
      const float* tb = ts + (wmh * 32 + l31) * PITCH + kpart * KPX + 4 * half;
#pragma unroll 2
      for (int q = 0; q < KPX / 8; ++q) {
        const float4 av = ld4(ga + 8 * q);
        const float4 bv = ld4(tb + 8 * q);
        dw2acc = mfma32(av.x, bv.x, dw2acc);
        dw2acc = mfma32(av.y, bv.y, dw2acc);
        dw2acc = mfma32(av.z, bv.z, dw2acc);
        dw2acc = mfma32(av.w, bv.w, dw2acc);
      }
    }
    __syncthreads();      // every wave is past its reads of t
    // ---- 6
#pragma unroll
    for (int m = 0; m < MH; ++m) {
      float dhv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        dhv[r] = accdt[m][r] * dgh[m][r];
        ts[(m * 32 + acc_row32(r, half)) * PITCH + n0 + l31] = dhv[r];
      }
      sdb1[m] += half_reduce16(dhv, lane);
    }
    __syncthreads();
    // ---- 7
    {
      f32x16 acc[MC];
#pragma unroll
      for (int m = 0; m < MC; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
      const float* hp = ts + half * PITCH + n0 + l31;
#pragma unroll
      for (int m = 0; m < MC; ++m) {
        const float* wp = w1s + half * W1P + m * 32 + l31;      // A[i = channel][k = hidden] = W1[hidden][channel]
#pragma unroll 8
        for (int s = 0; s < HID / 2; ++s) acc[m] = mfma32(wp[2 * s * W1P], hp[2 * s * PITCH], acc[m]);
      }
      const float* ga = ts + (wmh * 32 + l31) * PITCH + kpart * KPX + 4 * half;
      const float* ub = us + (wmc * 32 + l31) * PITCH + kpart * KPX + 4 * half;
#pragma unroll 2
      for (int q = 0; q < KPX / 8; ++q) {
        const float4 av = ld4(ga + 8 * q);
        const float4 bv = ld4(ub + 8 * q);
        dw1acc = mfma32(av.x, bv.x, dw1acc);
        dw1acc = mfma32(av.y, bv.y, dw1acc);
        dw1acc = mfma32(av.z, bv.z, dw1acc);
        dw1acc = mfma32(av.w, bv.w, dw1acc);
      }
      // (ds was last read before the barrier above)
#pragma unroll
      for (int m = 0; m < MC; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) bs[(m * 32 + acc_row32(r, half)) * PITCH + n0 + l31] = acc[m][r];
    }
    __syncthreads();
    // ---- 8  (the next commit writes u's tile, last read in step 7; v is written to this tile two barriers from here)
#pragma unroll
    for (int i = 0; i < PF::ITER; ++i) {
      const int idx = tid + i * NT;
      const int c = idx / (NPX / 4), q = idx % (NPX / 4);
      st4(a.du + off + (size_t)c * a.PW + 4 * q, ld4(bs + c * PITCH + 4 * q));
    }
  }

  // ---- partial slabs
  {
    const size_t slab = (size_t)blockIdx.x * KSPLIT + kpart;
    float* d1 = a.dw1_part + slab * HID * C;
    float* d2 = a.dw2_part + slab * C * HID;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      d1[(wmh * 32 + acc_row32(r, half)) * C + wmc * 32 + l31] = dw1acc[r];
      d2[(wmc * 32 + acc_row32(r, half)) * HID + wmh * 32 + l31] = dw2acc[r];
    }
  }
  if ((lane & 16) == 0) {      // lanes 16-31 / 48-63 hold duplicates
    const size_t slab = (size_t)blockIdx.x * 4 + wave;
    const int row = acc_row32(reduce16_id(lane), half);
#pragma unroll
    for (int m = 0; m < MH; ++m) a.db1_part[slab * HID + m * 32 + row] = sdb1[m];
#pragma unroll
    for (int m = 0; m < MC; ++m) a.db2_part[slab * C + m * 32 + row] = sdb2[m];
  }
  if (a.dg_part) {
#pragma unroll
    for (int i = 0; i < PF::ITER; ++i) {      // lanes 0-31 / 32-63 of a wave share one channel per pass
      const float s = half_reduce_sum(sdg[i]);
      if (l31 == 0) a.dg_part[(size_t)blockIdx.x * C + (tid + i * NT) / (NPX / 4)] = s;
    }
  }
}
