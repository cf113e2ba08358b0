// Domain padding of the FNO family (neuralop/models/padding.py:35-95; FNO.forward pads the lifted field by a fraction of the
// grid, runs the Fourier blocks on the extended grid and crops before the projection, tfno.py:195-211):
//   k_domain_pad   y (planes, R0, R1, R2) = x (planes, I0, I1, I2) set into zeros, `before[d]` zeros in front of axis d
//   k_domain_crop  x = the interior of y
// Each is the other's adjoint, so the two serve all four directions.  Pure data movement, bound by memory:
//   - the work is laid over the flattened OUTPUT in quads of four floats that start on 16-byte boundaries of the output's
//     address, so every store of the loop is one whole 16-byte vector whatever the row lengths are (41 -> 45, 73, 80: rows
//     are rarely multiples of four floats, and a quad may run over a row end or a plane end); the up to three elements in
//     front of the first boundary and behind the last whole quad are written one by one by the grid's last thread;
//   - the input is the side that cannot be aligned as well: a quad that lies in one input row on a 16-byte boundary is one
//     vector load, any other takes four scalar loads;
//   - a thread decomposes its first quad's offset into (plane, i0, i1, i2) once; from then on it adds the loop's stride, which
//     the host hands over already decomposed in the output's radices, and carries: no division inside the loop.
// Data travels as 32-bit words, never as floats: NaN payloads, infinities and -0.0 arrive bit for bit, and a margin is the
// word 0 = +0.0f.  No atomics, no workspace: the launch can be captured.  1-D and 2-D tensors are 3-D ones with leading
// extents of 1.
#pragma once
#include "fno_dev.h"

typedef unsigned dompad_u32x4 __attribute__((ext_vector_type(4)));      // one 16-byte access

struct DomPadArgs {
  const unsigned* in;
  unsigned* out;
  int R[3];          // output extents
  int I[3];          // input extents
  int off[3];        // input coordinate = output coordinate + off  (pad: -before, crop: +before)
  int s[3];          // the loop's stride (4 * threads of the grid, in elements) decomposed in the radices R ...
  long long sp;      // ... and its plane part
  long long nq;      // whole 16-byte quads of the output
  long long n_out;   // output elements
  int head;          // output elements in front of the first 16-byte boundary (0..3)
};

// the word at output coordinates (p, i0, i1, i2): the input's where they fall inside it, else 0 (only a pad has an outside)
template <bool PAD>
FNO_DEV unsigned dompad_fetch(const DomPadArgs& a, long long p, int i0, int i1, int i2) {
  const int c0 = i0 + a.off[0], c1 = i1 + a.off[1], c2 = i2 + a.off[2];
  if (PAD && ((unsigned)c0 >= (unsigned)a.I[0] || (unsigned)c1 >= (unsigned)a.I[1] || (unsigned)c2 >= (unsigned)a.I[2])) return 0u;
  return a.in[((p * a.I[0] + c0) * a.I[1] + c1) * a.I[2] + c2];
}

// one output element by its flat offset (the few in front of and behind the quads: divisions are fine here)
template <bool PAD>
FNO_DEV void dompad_edge(const DomPadArgs& a, long long e) {
  long long r = e;
  const int i2 = (int)(r % a.R[2]); r /= a.R[2];
  const int i1 = (int)(r % a.R[1]); r /= a.R[1];
  const int i0 = (int)(r % a.R[0]); r /= a.R[0];
  a.out[e] = dompad_fetch<PAD>(a, r, i0, i1, i2);
}

template <bool PAD>
FNO_DEV void dompad_body(const DomPadArgs& a) {
  const long long nthr = (long long)gridDim.x * 256;
  long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q == nthr - 1) {
    for (long long e = 0; e < a.head; ++e) dompad_edge<PAD>(a, e);
    for (long long e = a.head + 4 * a.nq; e < a.n_out; ++e) dompad_edge<PAD>(a, e);
  }
  if (q >= a.nq) return;
  const int R0 = a.R[0], R1 = a.R[1], R2 = a.R[2], I0 = a.I[0], I1 = a.I[1], I2 = a.I[2];
  long long e = a.head + 4 * q, p = e;
  int i2 = (int)(p % R2); p /= R2;
  int i1 = (int)(p % R1); p /= R1;
  int i0 = (int)(p % R0); p /= R0;
  const long long step = 4 * nthr;
  for (; q < a.nq; q += nthr, e += step) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (i2 + 3 < R2) {      // the quad lies in one output row
      const int c0 = i0 + a.off[0], c1 = i1 + a.off[1], c2 = i2 + a.off[2];
      const bool row = !PAD || ((unsigned)c0 < (unsigned)I0 && (unsigned)c1 < (unsigned)I1);
      if (row && (!PAD || (c2 + 3 >= 0 && c2 < I2))) {
        const unsigned* base = a.in + ((p * I0 + c0) * I1 + c1) * I2;      // the input row (c0, c1): inside the input
        const bool whole = !PAD || (c2 >= 0 && c2 + 3 < I2);                 // all four words lie in it
        if (whole && ((uintptr_t)(base + c2) & 15) == 0) {
          // (a native vector type: the struct copy of a uint4 is split into four word loads, which the compiler then folds
          // into the scalar arm below where the two arms read the same words - the crop - and the 16-byte load is gone)
          const dompad_u32x4 t = *reinterpret_cast<const dompad_u32x4*>(base + c2);
          v = make_uint4(t.x, t.y, t.z, t.w);
        } else {             // an address is formed only for a word that lies in the row
          if (!PAD || (unsigned)c2 < (unsigned)I2) v.x = base[c2];
          if (!PAD || (unsigned)(c2 + 1) < (unsigned)I2) v.y = base[c2 + 1];
          if (!PAD || (unsigned)(c2 + 2) < (unsigned)I2) v.z = base[c2 + 2];
          if (!PAD || (unsigned)(c2 + 3) < (unsigned)I2) v.w = base[c2 + 3];
        }
      }
    } else {                // it runs over a row end (and perhaps a plane end): walk it element by element
      long long wp = p;
      int w0 = i0, w1 = i1, w2 = i2;
      unsigned w[4];
      for (int k = 0; k < 4; ++k) {
        w[k] = dompad_fetch<PAD>(a, wp, w0, w1, w2);
        if (++w2 == R2) {
          w2 = 0;
          if (++w1 == R1) {
            w1 = 0;
            if (++w0 == R0) { w0 = 0; ++wp; }
          }
        }
      }
      v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    dompad_u32x4 o;
    o.x = v.x; o.y = v.y; o.z = v.z; o.w = v.w;
    *reinterpret_cast<dompad_u32x4*>(a.out + e) = o;
    // the next quad of this thread: add the decomposed stride, lowest digit first; every digit and every stride digit is
    // below its radix, so one carry per digit is all there can be
    i2 += a.s[2]; if (i2 >= R2) { i2 -= R2; ++i1; }
    i1 += a.s[1]; if (i1 >= R1) { i1 -= R1; ++i0; }
    i0 += a.s[0]; if (i0 >= R0) { i0 -= R0; ++p; }
    p += a.sp;
  }
}

__global__ void __launch_bounds__(256) k_domain_pad(DomPadArgs a) { dompad_body<true>(a); }
__global__ void __launch_bounds__(256) k_domain_crop(DomPadArgs a) { dompad_body<false>(a); }
