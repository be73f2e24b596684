// idf_cdf_fast.h -- the decoders' few-instruction forms of idf::rans_cdf (idf_cdf.h), device
// only: bit-identical to it on the operands the decoders produce (the conditions are stated at
// each function).  Shared by rans_kernels.hip (the flow's streams) and predict_kernels.hip (the
// predictive streams of escaped tiles).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "idf_cdf.h"

#pragma clang fp contract(off)

namespace idf {

// ---- bit-exact CDF with the divisions in their unscaled form.
// hipcc lowers a f64 division x / y to v_div_scale (x2), v_rcp + two Newton steps on the
// scaled y, q = x * r, a residual FMA, v_div_fmas and v_div_fixup.  For the operands the
// coder produces (float inputs widened to double, |quotient| far inside the double
// range, finite nonzero y) div_scale leaves both operands unchanged (VCC = 0), div_fmas
// is a plain FMA and div_fixup returns its input, so the same arithmetic without them is
// bit-identical; the y-only half (the refined reciprocal) is hoisted per symbol.
__device__ __forceinline__ double rcp_refined(double y) {
  double r = __builtin_amdgcn_rcp(y);
  r = __builtin_fma(r, __builtin_fma(-y, r, 1.0), r);
  return __builtin_fma(r, __builtin_fma(-y, r, 1.0), r);
}
__device__ __forceinline__ double div_unscaled(double x, double y, double r) {
  const double q = x * r;
  return __builtin_fma(__builtin_fma(-y, q, x), r, q);
}
// scale range in which the hoisted division is used (else rans_cdf's own '/')
__device__ __forceinline__ bool fast_scale_ok(float scale) {
  return scale >= 0x1p-60f && scale <= 0x1p60f;
}

// part1 = round((M - 2048) / (1 + expf(-u))) of rans.pyx:34 as a function of the float
// logistic argument u alone, in few instructions (the decoder's serial chain is issue-bound:
// one wave, one instruction per ~4 cycles):
//   * glibc expf's table path on x = -u clamped to [-0x1.9fe368p6, 0x1.62e42ep6] (one
//     v_med3): outside that range glibc returns 0 (below) or inf (above), and the clamp ends
//     give the same part1 through the table path -- expf(lo) is below 2^-53, so 1 + expf
//     rounds to 1 and part1 = M - 2048; expf(hi) is ~2^128, so part1 rounds to 0;
//   * 1/y by v_rcp_f64, ONE Newton step and the quotient correction (the IEEE division
//     hipcc emits takes two Newton steps, div_scale and div_fixup);
//   * roundf(p) for p >= 0 as v_cvt_rpi_i32_f32 (floor(p + 0.5) without rounding the sum).
// Equal to part1_ref (the reference's arithmetic) on every non-NaN float u
// (idf_rans_part1_selfcheck: all 2^32 bit patterns); u is never NaN here (scale > 0).
__device__ __forceinline__ int part1_ref(float u, const uint64_t* tab) {
  const double l = 1.0 / (1.0 + (double)expf_glibc(-u, tab));
  return (int)round_f((float)(l * 16775168.0));
}
__device__ __forceinline__ int part1_fast(float u, const uint64_t* tab) {
  const double InvLn2N = 0x1.71547652b82fep+0 * 32;
  const double SHIFT = 0x1.8p+52;
  const double C0 = 0x1.c6af84b912394p-5 / (32.0 * 32.0 * 32.0);
  const double C1 = 0x1.ebfce50fac4f3p-3 / (32.0 * 32.0);
  const double C2 = 0x1.62e42ff0c52d6p-1 / 32.0;
  const float x = __builtin_amdgcn_fmed3f(-u, -0x1.9fe368p6f, 0x1.62e42ep6f);
  const double xd = (double)x;
  double kd = __builtin_fma(InvLn2N, xd, SHIFT);
  const uint64_t ki = d2u(kd);
  kd -= SHIFT;
  const double r = __builtin_fma(InvLn2N, xd, -kd);
  const double sc = u2d(tab[ki % 32] + (ki << 47));
  const double z = __builtin_fma(C0, r, C1);
  const double r2 = r * r;
  double ey = __builtin_fma(C2, r, 1.0);
  ey = __builtin_fma(z, r2, ey);
  const double y = 1.0 + (double)(float)(ey * sc);
  double rc = __builtin_amdgcn_rcp(y);
  rc = __builtin_fma(rc, __builtin_fma(-y, rc, 1.0), rc);
  const double l = __builtin_fma(__builtin_fma(-y, rc, 1.0), rc, rc);  // 1/y, correctly rounded
  const float p = (float)(l * 16775168.0);
  int pn;
  asm("v_cvt_rpi_i32_f32 %0, %1" : "=v"(pn) : "v"(p));
  return pn;
}
// The exact CDF at bin q (x = q/256) for scale > 0 with fast_scale_ok(scale): rans_cdf_rs with
// the integer-exact forms of its x terms -- part2 = round((x - lower_f) * 256) + 1 = q - lower + 1
// (both operands are multiples of 2^-8: the f32 subtraction is exact), (double)x + 2^-9 =
// (2q + 1) * 2^-9 (exact, so fma((2q + 1), 2^-9, -mean) is the reference's rounded difference)
// -- and part1_fast.
__device__ __forceinline__ int cdf_bin(int q, int lower, double mean_d, double scale_d, double rs,
                                       const uint64_t* tab) {
  // (2q + 1) * 2^-9 is exact, so one fma rounds exactly as the reference's subtraction
  const double t = __builtin_fma((double)(2 * q + 1), 0.001953125, -mean_d);
  const float u = (float)div_unscaled(t, scale_d, rs);
  return part1_fast(u, tab) + (q - lower + 1);
}

}  // namespace idf
