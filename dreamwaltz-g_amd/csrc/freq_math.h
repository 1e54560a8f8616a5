// freq_math.h -- the frequency encoding of a direction (boundary B22: the learned background's encoder_bg), written once for the HIP
// kernels (nerf_background.hip) and compilable by a C compiler for the host (tests/hostmath/freq_math_host.c).
//
//   freq_output_dim     3 + 6 degree: FreqEncoder.output_dim for input_dim 3
//   freq_column         column c of the encoding of x[3]
//   freq_encode         all 3 + 6 degree columns
// The layout is the reference FreqEncoder's: out[c] = x[c] for c < 3; for c >= 3, c = 3 + (2 f + s) * 3 + d holds sin(2^f x[d]) for
// s = 0 and cos(2^f x[d]) for s = 1, f < degree.  The scale by 2^f is scalbnf (exact); the functions are sinf and cosf proper -- the
// reference's kernel takes a fast-intrinsic sine of x + phase and a rounded pi / 2 shift for the cosine, which is not restated: parity is
// to the mathematical value.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DWG_FREQ_HD __host__ __device__ __forceinline__
#else
#define DWG_FREQ_HD static inline
#endif

#define DWG_FREQ_MAX_DEGREE 8u       /* 2^7 |x| <= 128 for a unit direction; output width at most 51 */

DWG_FREQ_HD uint32_t freq_output_dim(uint32_t degree) { return 3u + 6u * degree; }

DWG_FREQ_HD float freq_column(const float* x, uint32_t c) {
    if (c < 3u) return x[c];
    const uint32_t e = c - 3u, j = e / 3u, d = e - 3u * j;     // j = 2 f + s
    const float v = scalbnf(x[d], (int)(j >> 1));
    return (j & 1u) ? cosf(v) : sinf(v);
}

DWG_FREQ_HD void freq_encode(const float* x, uint32_t degree, float* out) {
    const uint32_t n = freq_output_dim(degree);
    for (uint32_t c = 0; c < n; ++c) out[c] = freq_column(x, c);
}
