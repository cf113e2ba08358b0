// Device-resident PINO training data (libs/pino_utils/datasets.py DevicePinoBatches): the tensors of a
// MultipleReynoldsKFaDataset stay on the device and a batch (u, a_in) is two launches:
//   k_data_transpose_gather   out[e * out_stride + c * rows + r] = src[idx[e] * rows * cols + r * cols + c]
//                             (the dataset hands u out as a permuted view of (N, T, S, S) storage: rows = T, cols = S * S)
//   k_pino_input              out[e, x, y, k, :] = (gx[x], gy[y], gt[k], a0[idx[e], x, y])     channels-last (count, s1, s2, t, 4)
// Both move 32-bit words, never floats: NaN payloads, infinities, -0.0 and denormals arrive bit for bit (k_domain_pad.h).
// The transpose: a workgroup takes TG_COLS columns of one entry.  The source is read along c, a 16-byte load per lane where the
// address allows it, 16 consecutive lanes on the 256 contiguous bytes of a row; the layout turns in LDS; the destination - the
// TG_COLS * rows contiguous floats of the column block - is laid over its own ADDRESS in 16-byte quads (k_data_gather.h): every
// store of the loop is one whole vector along r at any (odd) `rows`, the up to three floats in front of the first boundary and
// behind the last whole quad are written one by one.
// LDS: word (row lr, column c) of the tile lives at slot(lr) * TG_PITCH + col(c) with slot(lr) = (lr & 3) * 32 + (lr >> 2),
// col(c) = 9 c mod 64 and the odd pitch 65, so a row starts on bank lr >> 2 of the 32 a 4-byte access sees.  Writing, the 16
// lanes of a row put word j of their quads on banks (lr >> 2) + 4 i + 9 j, two lanes per bank, and the two rows of a 32-lane
// half are rows lr and lr + 4, one bank apart: two lanes per bank in all, free for a 4-byte write.  Reading, the lanes of a
// wave hold consecutive quads of a column, rows r0 + 4 i + j: slots that follow each other, 65 words apart - 32 different
// banks within a column.  A group of 32 lanes covers 128 floats, so at rows = 65 it always runs over a column's end; the next
// column's lanes restart 16 banks back, and col() moves them on by 9: one bank with two lanes per group at rows 65, 33 and 9
// (with col(c) = c: three to five lanes), none where a group stays inside a column.
// More rows than the tile holds (TG_ROWS): chunks of TG_OWN rows.  A quad belongs to the chunk of its first row; a chunk loads
// the TG_OWN + 3 rows its quads can reach and, where they run over the end of a column, rows 0..2 for the next column's start.
// Addressing is 64-bit.  An index is compared unsigned against n_src BEFORE it becomes an address; an entry out of range reads
// nothing and is filled with NaN (the contract of fno_data_gather).  No atomics, no workspace: the launches can be captured.
#pragma once
#include "fno_dev.h"

typedef unsigned pbatch_u32x4 __attribute__((ext_vector_type(4)));       // one 16-byte access

#define TG_COLS 64        // columns of a tile: 256 contiguous source bytes per row
#define TG_PITCH 65       // words between two row slots (odd)
#define TG_ROWS 128       // row slots of the tile
#define TG_OWN 120        // rows a chunk owns when rows > TG_ROWS; it loads TG_OWN + 3 and up to 3 wrapped rows: 126 slots
#define PBATCH_NAN 0x7fc00000u

struct TransposeGatherArgs {
  const unsigned* src;
  const long long* idx;
  unsigned* out;
  unsigned long long n_src, out_stride, count;
  int rows, cols;
};

FNO_DEV int tg_slot(int lr) { return ((lr & 3) << 5) + (lr >> 2); }
FNO_DEV int tg_col(int cl) { return (9 * cl) & (TG_COLS - 1); }           // where column cl of the tile lives in a row slot

// the word of (column cl of the tile, row r of the entry), r possibly past the column's end: it then belongs to a later column
FNO_DEV unsigned tg_word(const unsigned* tile, int cl, unsigned r, unsigned rows, int first, bool chunked) {
  while (r >= rows) { r -= rows; ++cl; }
  const int lr = !chunked ? (int)r : r >= (unsigned)first ? (int)r - first : TG_OWN + 3 + (int)r;
  return tile[tg_slot(lr) * TG_PITCH + tg_col(cl)];
}

__global__ void __launch_bounds__(256) k_data_transpose_gather(TransposeGatherArgs a) {
  __shared__ unsigned tile[TG_ROWS * TG_PITCH];
  const unsigned rows = (unsigned)a.rows;
  const int cols = a.cols, tid = threadIdx.x;
  const int c0 = (int)blockIdx.x * TG_COLS;                              // (the host sizes grid.x to the column blocks)
  const int n = min(TG_COLS, cols - c0);
  const bool chunked = rows > TG_ROWS;
  const int nchunk = chunked ? (int)((rows + TG_OWN - 1) / TG_OWN) : 1;
  const unsigned long long len = (unsigned long long)n * rows;           // floats of this column block, contiguous in the output
  // loading: quad of the row, and the row of the pass of 16 - the two rows of a 32-lane half are four apart (0, 4, 1, 5, ..)
  const int qc = tid & 15, w = tid >> 4, rl = (w & 1) * 4 + ((w >> 1) & 3) + (w & 8);
  const unsigned step_c = 1024u / rows, step_r = 1024u % rows;           // the store loop's stride of 256 quads in (column, row)
  for (unsigned long long e = blockIdx.y; e < a.count; e += gridDim.y) {
    const unsigned long long s = (unsigned long long)a.idx[e];
    const bool live = s < a.n_src;                                       // unsigned: a negative index is out of range too
    const unsigned* plane = a.src + (live ? s : 0ull) * rows * (unsigned long long)cols;
    unsigned* o = a.out + e * a.out_stride + (unsigned long long)c0 * rows;
    const unsigned long long head = len < 4 ? 0 : (unsigned long long)((4 - (((uintptr_t)o >> 2) & 3)) & 3);
    const unsigned long long nq = (len - head) / 4;
    for (int j = 0; j < nchunk; ++j) {
      const int first = j * TG_OWN;                                      // first row of the chunk
      const int nmain = chunked ? min(TG_OWN + 3, (int)rows - first) : (int)rows;
      const bool wrap = chunked && (long long)first + TG_OWN + 3 >= (long long)rows;      // its quads can run into the next column
      if (live) {
        const int nload = wrap ? TG_OWN + 6 : nmain;
        for (int lr = rl; lr < nload; lr += 16) {
          if (lr >= nmain && lr < TG_OWN + 3) continue;
          const int r = lr < nmain ? first + lr : lr - (TG_OWN + 3);
          const int c = c0 + 4 * qc;
          const unsigned* p = plane + (unsigned long long)r * cols + c;
          unsigned* t = tile + tg_slot(lr) * TG_PITCH;
          if (c + 3 < cols && ((uintptr_t)p & 15) == 0) {
            const pbatch_u32x4 v = *reinterpret_cast<const pbatch_u32x4*>(p);
            t[tg_col(4 * qc)] = v.x; t[tg_col(4 * qc + 1)] = v.y; t[tg_col(4 * qc + 2)] = v.z; t[tg_col(4 * qc + 3)] = v.w;
          } else {                                                        // an address is formed only for a word of the row
            for (int k = 0; k < 4; ++k)
              if (c + k < cols) t[tg_col(4 * qc + k)] = p[k];
          }
        }
      }
      __syncthreads();
      if (tid < 6) {      // the floats outside the whole quads: three in front, three behind
        const unsigned long long k = tid < 3 ? (unsigned long long)tid : head + 4 * nq + (tid - 3);
        if (tid < 3 ? k < head : k < len) {
          const int cl = (int)(k / rows);
          const unsigned r = (unsigned)(k - (unsigned long long)cl * rows);
          if (!chunked || (int)(r / TG_OWN) == j) o[k] = live ? tg_word(tile, cl, r, rows, first, chunked) : PBATCH_NAN;
        }
      }
      if ((unsigned long long)tid < nq) {
        const unsigned long long k0 = head + 4ull * tid;
        int cl = (int)(k0 / rows);
        unsigned r = (unsigned)(k0 - (unsigned long long)cl * rows);
        for (unsigned long long q = tid; q < nq; q += 256) {
          if (!chunked || (int)(r / TG_OWN) == j) {
            pbatch_u32x4 v = {PBATCH_NAN, PBATCH_NAN, PBATCH_NAN, PBATCH_NAN};
            if (live) {
              v.x = tg_word(tile, cl, r, rows, first, chunked);
              v.y = tg_word(tile, cl, r + 1, rows, first, chunked);
              v.z = tg_word(tile, cl, r + 2, rows, first, chunked);
              v.w = tg_word(tile, cl, r + 3, rows, first, chunked);
            }
            *reinterpret_cast<pbatch_u32x4*>(o + head + 4 * q) = v;
          }
          r += step_r; cl += (int)step_c;
          if (r >= rows) { r -= rows; ++cl; }
        }
      }
      __syncthreads();      // the tile is loaded again: by the next chunk or the next entry
    }
  }
}

#define PIN_POINTS 32     // (x, y) points of a workgroup: 32 * t whole 16-byte stores, the a0 word of a point read once

struct PinoInputArgs {
  const unsigned* a0;
  const long long* idx;
  const unsigned *gx, *gy, *gt;
  unsigned* out;
  unsigned long long n_src, count, npts;      // npts = s1 * s2
  int s2, t;
};

__global__ void __launch_bounds__(256) k_pino_input(PinoInputArgs a) {
  __shared__ unsigned sx[PIN_POINTS], sy[PIN_POINTS], sa[PIN_POINTS];
  const int tid = threadIdx.x;
  const unsigned t = (unsigned)a.t;
  const unsigned step_p = 256u / t, step_k = 256u % t;
  const unsigned long long nblk = (a.npts + PIN_POINTS - 1) / PIN_POINTS;
  for (unsigned long long e = blockIdx.y; e < a.count; e += gridDim.y) {
    const unsigned long long s = (unsigned long long)a.idx[e];
    const bool live = s < a.n_src;                                       // unsigned: a negative index is out of range too
    const unsigned* plane = a.a0 + (live ? s : 0ull) * a.npts;
    for (unsigned long long b = blockIdx.x; b < nblk; b += gridDim.x) {
      const unsigned long long p0 = b * PIN_POINTS;
      const int np = (int)min((unsigned long long)PIN_POINTS, a.npts - p0);
      if (tid < np) {
        const unsigned long long p = p0 + tid, x = p / (unsigned)a.s2;
        sx[tid] = a.gx[x];
        sy[tid] = a.gy[p - x * (unsigned)a.s2];
        sa[tid] = live ? plane[p] : PBATCH_NAN;
      }
      __syncthreads();
      // consecutive lanes write consecutive k, then y: a wave writes 1 KB of whole lines
      pbatch_u32x4* o = reinterpret_cast<pbatch_u32x4*>(a.out) + (e * a.npts + p0) * t;
      const unsigned long long total = (unsigned long long)np * t;
      unsigned pt = (unsigned)tid / t, k = (unsigned)tid - pt * t;
      for (unsigned long long i = tid; i < total; i += 256) {
        pbatch_u32x4 v;
        v.x = sx[pt]; v.y = sy[pt]; v.z = a.gt[k]; v.w = sa[pt];
        if (!live) v.x = v.y = v.z = PBATCH_NAN;
        o[i] = v;
        k += step_k; pt += step_p;
        if (k >= t) { k -= t; ++pt; }
      }
      __syncthreads();
    }
  }
}
