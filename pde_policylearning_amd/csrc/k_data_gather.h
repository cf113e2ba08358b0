// Device-resident training data (libs/pde_data_loader.py DeviceBatches): the raw snapshots of a folder
// stay on the device in their file dtype and a batch is assembled from them in one launch per tensor:
//   k_data_gather   out[e * out_stride + i * cols + j] = float( f( src[idx[e] * snap_elems + offset + i * row_stride + j * col_stride] ) )
// with f the identity (gather and cast) or NormalizerGivenMeanStd.encode, (x - mean[i][j]) / (std[i][j] + eps), in the type
// torch's promotion gives the host expression: float64 when the snapshots or the statistics are float64, float32 when both
// are float32.  Every operation is rounded once (a true division: the build has no fast-math and fp32 division is correctly
// rounded by default), `std + eps` is formed in the statistics' own type as `tensor + python_float` forms it, and one last
// rounding makes the float32 result - the bits of `encode(...)` on the host followed by `.float()` on the device.
// The one strided view covers downsample + crop (row_stride = d * C0, col_stride = d), a plane V[:, p, :] (offset = p * Nz,
// row_stride = Ny * Nz), a whole field, and one target plane of a (T, P, X, Z) tensor (out advanced, out_stride = P * X * Z).
//   - the work of an entry is laid over its OUTPUT in quads of four floats that start on 16-byte boundaries of the output's
//     address (k_domain_pad.h): every store of the loop is one whole 16-byte vector at any `cols` and any `out_stride`; the up
//     to three elements in front of the first boundary and behind the last whole quad are written one by one;
//   - a quad that lies in one source row with col_stride == 1 on a 16-byte boundary is read with 16-byte loads, any other with
//     four scalar loads; consecutive threads read consecutive quads, so unit-stride rows are read in whole cache lines.  Plain
//     (temporal) loads: the pool is read again every epoch;
//   - all address arithmetic is 64-bit (a pool may exceed 4 GB); an index is compared unsigned against n_src BEFORE it is
//     multiplied into an address, and an entry whose index is out of range reads nothing and is filled with NaN: no buffer
//     content can become an out-of-bounds address.
// No atomics, no workspace, nothing allocated: the launch can be captured.
#pragma once
#include "fno_dev.h"

typedef float dgather_f32x4 __attribute__((ext_vector_type(4)));       // one 16-byte access
typedef double dgather_f64x2 __attribute__((ext_vector_type(2)));

struct DataGatherArgs {
  const void* src;
  const long long* idx;
  const void *mean, *sd;                  // (rows, cols) contiguous, of the statistics' type; unused by the cast-only kernels
  float* out;
  unsigned long long n_src, snap_elems, offset, row_stride, col_stride, out_stride, count;
  long long n;                            // rows * cols
  int cols;
  double eps;
};

// encode in the promoted type, one rounding per operation, one to float32 at the end
FNO_DEV float dgather_encode(float x, float m, float s, double eps) { return (x - m) / (s + (float)eps); }
FNO_DEV float dgather_encode(double x, float m, float s, double eps) { return (float)((x - (double)m) / (double)(s + (float)eps)); }
FNO_DEV float dgather_encode(float x, double m, double s, double eps) { return (float)(((double)x - m) / (s + eps)); }
FNO_DEV float dgather_encode(double x, double m, double s, double eps) { return (float)((x - m) / (s + eps)); }

// (row, column) of the flat offset k inside an entry; planes below 2^32 points take the 32-bit division
FNO_DEV void dgather_split(long long k, int cols, long long& i, int& j) {
  if (k <= 0xffffffffll) {
    const unsigned q = (unsigned)k / (unsigned)cols;
    i = q;
    j = (int)((unsigned)k - q * (unsigned)cols);
  } else {
    i = k / cols;
    j = (int)(k - i * cols);
  }
}

template <typename S, typename M, bool NORM>
FNO_DEV float dgather_finish(const DataGatherArgs& a, S x, long long k) {
  if (!NORM) return (float)x;
  return dgather_encode(x, static_cast<const M*>(a.mean)[k], static_cast<const M*>(a.sd)[k], a.eps);
}

// four consecutive source elements from a 16-byte boundary
FNO_DEV void dgather_load4(const float* p, float* x) {
  const dgather_f32x4 t = *reinterpret_cast<const dgather_f32x4*>(p);
  x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
}
FNO_DEV void dgather_load4(const double* p, double* x) {
  const dgather_f64x2 t = *reinterpret_cast<const dgather_f64x2*>(p), u = *reinterpret_cast<const dgather_f64x2*>(p + 2);
  x[0] = t.x; x[1] = t.y; x[2] = u.x; x[3] = u.y;
}

template <typename S, typename M, bool NORM>
__global__ void __launch_bounds__(256) k_data_gather(DataGatherArgs a) {
  const long long nthr = (long long)gridDim.x * 256;
  const int cols = a.cols;
  const float fill = __builtin_nanf("");
  for (unsigned long long e = blockIdx.y; e < a.count; e += gridDim.y) {
    float* o = a.out + e * a.out_stride;
    const unsigned long long s = (unsigned long long)a.idx[e];
    const bool live = s < a.n_src;            // unsigned: a negative index is out of range too
    const S* snap = static_cast<const S*>(a.src) + (live ? s : 0ull) * a.snap_elems + a.offset;
    const long long head = a.n < 4 ? 0 : (long long)((4 - (((uintptr_t)o >> 2) & 3)) & 3);
    const long long nq = (a.n - head) / 4;
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x < 6) {      // the elements outside the whole quads: three in front, three behind
      const long long k = threadIdx.x < 3 ? (long long)threadIdx.x : head + 4 * nq + (threadIdx.x - 3);
      if (threadIdx.x < 3 ? k < head : k < a.n) {
        float v = fill;
        if (live) {
          long long i;
          int j;
          dgather_split(k, cols, i, j);
          v = dgather_finish<S, M, NORM>(a, snap[(unsigned long long)i * a.row_stride + (unsigned long long)j * a.col_stride], k);
        }
        o[k] = v;
      }
    }
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < nq; q += nthr) {
      const long long k = head + 4 * q;
      dgather_f32x4 v = {fill, fill, fill, fill};
      if (live) {
        long long i;
        int j;
        dgather_split(k, cols, i, j);
        S x[4];
        const S* row = snap + (unsigned long long)i * a.row_stride;
        if (j + 3 < cols) {      // the quad lies in one row
          const S* p = row + (unsigned long long)j * a.col_stride;
          if (a.col_stride == 1 && ((uintptr_t)p & 15) == 0) {
            dgather_load4(p, x);
          } else {
            x[0] = p[0]; x[1] = p[a.col_stride]; x[2] = p[2 * a.col_stride]; x[3] = p[3 * a.col_stride];
          }
        } else {                 // it runs over a row end (rows may be shorter than a quad): walk it
          for (int c = 0; c < 4; ++c) {
            x[c] = row[(unsigned long long)j * a.col_stride];
            if (++j == cols) { j = 0; row += a.row_stride; }
          }
        }
        v.x = dgather_finish<S, M, NORM>(a, x[0], k);
        v.y = dgather_finish<S, M, NORM>(a, x[1], k + 1);
        v.z = dgather_finish<S, M, NORM>(a, x[2], k + 2);
        v.w = dgather_finish<S, M, NORM>(a, x[3], k + 3);
      }
      *reinterpret_cast<dgather_f32x4*>(o + k) = v;
    }
  }
}
