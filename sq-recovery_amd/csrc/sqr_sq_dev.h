// Device-inline superquadric math of one voxel, point or ray, shared by the losses and renders (sqr_loss.hip)
// and the classical fitting stack (sqr_fit.hip).  Reference algorithm (timoblak/sq-recovery, torch/):
//   clamps             classes.py:224-230 (a in [.05,1], e in [.1,1], t in [0,1]; q untouched)
//   rotation           quaternion.py:19-21 (conjugate), :46-67 (mat_from_quaternion, not normalised)
//   inside-outside     classes.py:246-273: v = Rc (g - t); u = v/a; A1=u0^2 ... (exact 0 -> 1e-4);
//                      A=A1^(1/e2), B=B1^(1/e2), C=C1^(1/e1), E=(A+B)^(e2/e1), G=(E+C)^e1
// The pow chain is evaluated in the log2 domain
// (lA = log2(A1)/e2, log2(A+B) = max + log2(1 + 2^-|d|), ...) so nothing under/overflows in
// fp32 where the reference's float64 does not, and every ratio the backward needs (A/F1, C/F/C1,
// ...) is a single exp2 of a difference of logs.
#pragma once
#include <float.h>
#include <math.h>

namespace sqr {

constexpr float kLn2 = 0.69314718055994530942f;
constexpr float kLog2e = 1.44269504088896340736f;

__device__ __forceinline__ float fexp2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float flog2(float x) { return __builtin_amdgcn_logf(x); }
__device__ __forceinline__ float frcp(float x) { return __builtin_amdgcn_rcpf(x); }

// torch.clamp semantics: NaN propagates; backward mask lo <= x <= hi (inclusive)
__device__ __forceinline__ float clampf(float x, float lo, float hi) {
  return x < lo ? lo : (x > hi ? hi : x);
}
__device__ __forceinline__ float inrange(float x, float lo, float hi) {
  return (x >= lo && x <= hi) ? 1.f : 0.f;
}

struct SQ {
  float a[3], ia[3];
  float e1, e2, ie1, ie2, r21;
  float t[3];
  float M[9];  // Rc = M(conj(q)), row-major
  float q[4];
  float mask[12];
};

// params -> clamped shape + rotation (classes.py:224-247, quaternion.py:19-67)
__device__ __forceinline__ void sq_load(const float* __restrict__ p, SQ& s) {
  float raw[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) raw[i] = p[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    s.a[i] = clampf(raw[i], 0.05f, 1.f);
    s.mask[i] = inrange(raw[i], 0.05f, 1.f);
    s.ia[i] = 1.f / s.a[i];
    s.t[i] = clampf(raw[5 + i], 0.f, 1.f);
    s.mask[5 + i] = inrange(raw[5 + i], 0.f, 1.f);
  }
  s.e1 = clampf(raw[3], 0.1f, 1.f);
  s.e2 = clampf(raw[4], 0.1f, 1.f);
  s.mask[3] = inrange(raw[3], 0.1f, 1.f);
  s.mask[4] = inrange(raw[4], 0.1f, 1.f);
  s.ie1 = 1.f / s.e1;
  s.ie2 = 1.f / s.e2;
  s.r21 = s.e2 / s.e1;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    s.q[i] = raw[8 + i];
    s.mask[8 + i] = 1.f;
  }
  const float x = -raw[8], y = -raw[9], z = -raw[10], w = raw[11];
  const float tx = 2.f * x, ty = 2.f * y, tz = 2.f * z;
  const float twx = tx * w, twy = ty * w, twz = tz * w;
  const float txx = tx * x, txy = ty * x, txz = tz * x;
  const float tyy = ty * y, tyz = tz * y, tzz = tz * z;
  s.M[0] = 1.f - (tyy + tzz); s.M[1] = txy - twz;         s.M[2] = txz + twy;
  s.M[3] = txy + twz;         s.M[4] = 1.f - (txx + tzz); s.M[5] = tyz - twx;
  s.M[6] = txz - twy;         s.M[7] = tyz + twx;         s.M[8] = 1.f - (txx + tyy);
}

struct Vox {
  float u0, u1, u2;
  float lA1, lB1, lC1;  // log2 of the (zero-fixed) squares
  float lA, lB, lC, lF1, lE, lF;
  float G;
  float rA, rB, rE, rC;  // A/F1, B/F1, E/F, C/F (the Jacobian's ratios)
};

// log2(2^x + 2^y) and the two shares 2^x / (2^x + 2^y), 2^y / (2^x + 2^y): one exp2, one log2 and
// one rcp (the shares come from e = 2^(min - max): 1 / (1 + e) and e / (1 + e))
__device__ __forceinline__ float lse2(float x, float y, float* sx, float* sy) {
  const float m = fmaxf(x, y);
  const float e = fexp2(fminf(x, y) - m);
  const float big = frcp(1.f + e), small = e * big;
  *sx = x >= y ? big : small;
  *sy = x >= y ? small : big;
  return m + flog2(1.f + e);
}

// classes.py:247-273 for one voxel; (dx,dy,dz) = g - t
__device__ __forceinline__ void vox_fwd(const SQ& s, float dx, float dy, float dz, Vox& f) {
  const float v0 = fmaf(s.M[0], dx, fmaf(s.M[1], dy, s.M[2] * dz));
  const float v1 = fmaf(s.M[3], dx, fmaf(s.M[4], dy, s.M[5] * dz));
  const float v2 = fmaf(s.M[6], dx, fmaf(s.M[7], dy, s.M[8] * dz));
  f.u0 = v0 * s.ia[0];
  f.u1 = v1 * s.ia[1];
  f.u2 = v2 * s.ia[2];
  float A1 = f.u0 * f.u0, B1 = f.u1 * f.u1, C1 = f.u2 * f.u2;
  A1 = (A1 == 0.f) ? 1e-4f : A1;  // classes.py:261-263
  B1 = (B1 == 0.f) ? 1e-4f : B1;
  C1 = (C1 == 0.f) ? 1e-4f : C1;
  f.lA1 = flog2(fmaxf(A1, FLT_MIN));
  f.lB1 = flog2(fmaxf(B1, FLT_MIN));
  f.lC1 = flog2(fmaxf(C1, FLT_MIN));
  f.lA = f.lA1 * s.ie2;
  f.lB = f.lB1 * s.ie2;
  f.lC = f.lC1 * s.ie1;
  f.lF1 = lse2(f.lA, f.lB, &f.rA, &f.rB);
  f.lE = s.r21 * f.lF1;
  f.lF = lse2(f.lE, f.lC, &f.rE, &f.rC);
  f.G = fexp2(s.e1 * f.lF);
}

// The per-ray form of vox_fwd for the ImplicitLoss walk: along a ray only gz varies, so
// u_i = ((M_i0 dx + M_i1 dy) + M_i2 (gz - t2)) / a_i = al_i + be_i gz (RayU, formed once per ray: three
// FMAs per voxel instead of twelve operations), and log2 A1 = 2 log2|u0| (no square, no FLT_MIN clamp:
// the zero fix of classes.py:261-263 applies exactly where the reference's fp32 square u0 * u0 is 0,
// i.e. |u0| <= 2^-75; between that and FLT_MIN^(1/2) u0^2 is a denormal whose true logarithm is kept).  lA..lC come out already divided by e2 / e1; the Jacobian needs
// 1/u_i (vox_jac11), not 2^-log2 A1.
constexpr float kSqZero = 0x1p-75f;  // largest |u| whose fp32 square is 0
struct RayU {
  float al[3], be[3];
  float lfixA, lfixB, lfixC;  // log2(1e-4) / e2, / e2, / e1 (the zero-fixed squares)
  float i2e2, i2e1;           // 2 / e2, 2 / e1
};
__device__ __forceinline__ void ray_u(const SQ& s, float dx, float dy, RayU& r) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float c = fmaf(s.M[3 * i], dx, fmaf(s.M[3 * i + 1], dy, -s.M[3 * i + 2] * s.t[2]));
    r.al[i] = c * s.ia[i];
    r.be[i] = s.M[3 * i + 2] * s.ia[i];
  }
  const float l4 = flog2(1e-4f);
  r.lfixA = l4 * s.ie2;
  r.lfixB = l4 * s.ie2;
  r.lfixC = l4 * s.ie1;
  r.i2e2 = 2.f * s.ie2;
  r.i2e1 = 2.f * s.ie1;
}
__device__ __forceinline__ void vox_fwd_ray(const SQ& s, const RayU& r, float gz, Vox& f) {
  f.u0 = fmaf(r.be[0], gz, r.al[0]);
  f.u1 = fmaf(r.be[1], gz, r.al[1]);
  f.u2 = fmaf(r.be[2], gz, r.al[2]);
  // the reference's fix applies where its fp32 square is 0: u * u rounds to +0 exactly when
  // |u| <= 2^-75 (u^2 <= 2^-150, half the smallest denormal; ties to even)
  f.lA = fabsf(f.u0) > kSqZero ? flog2(fabsf(f.u0)) * r.i2e2 : r.lfixA;
  f.lB = fabsf(f.u1) > kSqZero ? flog2(fabsf(f.u1)) * r.i2e2 : r.lfixB;
  f.lC = fabsf(f.u2) > kSqZero ? flog2(fabsf(f.u2)) * r.i2e1 : r.lfixC;
  f.lF1 = lse2(f.lA, f.lB, &f.rA, &f.rB);
  f.lE = s.r21 * f.lF1;
  f.lF = lse2(f.lE, f.lC, &f.rE, &f.rC);
  f.G = fexp2(s.e1 * f.lF);
}

// sigmoid(sharp (1-G)) and 1-sigmoid without cancellation
__device__ __forceinline__ void occupancy(float G, float sharp, float& occ, float& omo) {
  const float ex = fexp2(-sharp * (1.f - G) * kLog2e);
  occ = frcp(1.f + ex);
  omo = (ex < 1e30f) ? ex * occ : 1.f;
}

struct Moments {
  float m[17];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int i = 0; i < 17; ++i) m[i] = 0.f;
  }
};

// dL/docc at one voxel -> the 17 parameter moments (analytic bwd of classes.py:247-274):
//   m[0..2]  sum gu_i * u_i        (dL/da_i = -m_i / a_i)
//   m[3], m[4]  dL/de1, dL/de2 partials
//   m[5..7]  sum gu_i              (sum dL/dv_i = m / a_i)
//   m[8+3i+j] sum gu_i * g_j       (dL/dRc_ij = m/a_i - sum(dL/dv_i) t_j)
// (vox_bwd_lnG: from hG = dL/dln G on; vox_bwd: from dL/docc)
__device__ __forceinline__ void vox_bwd_lnG(const SQ& s, const Vox& f, float hG, float gx, float gy, float gz,
                                            Moments& M) {
  const float g_lnF = hG * s.e1;
  const float g_lnE = g_lnF * f.rE;
  const float g_lnC = g_lnF * f.rC;
  const float g_lnF1 = g_lnE * s.r21;
  const float rA = f.rA, rB = f.rB;
  const float g_lnA = g_lnF1 * rA, g_lnB = g_lnF1 * rB;
  // e1: lnG = e1 lnF ; lnE = (e2/e1) lnF1 ; lnC = lnC1/e1
  M.m[3] += kLn2 * (hG * f.lF - (g_lnE * f.lE + g_lnC * f.lC) * s.ie1);
  // e2: lnE ; lnA = lnA1/e2 ; lnB = lnB1/e2
  M.m[4] += kLn2 * s.ie2 * (g_lnE * f.lE - g_lnA * f.lA - g_lnB * f.lB);
  // u: d lnA1/du0 = 2 u0 / A1
  // (A / F1) / A1 etc.: the share times 2^-log2(A1) (A1 itself may sit below FLT_MIN)
  const float gu0 = 2.f * f.u0 * s.ie2 * g_lnF1 * rA * fexp2(-f.lA1);
  const float gu1 = 2.f * f.u1 * s.ie2 * g_lnF1 * rB * fexp2(-f.lB1);
  const float gu2 = 2.f * f.u2 * s.ie1 * g_lnF * f.rC * fexp2(-f.lC1);
  M.m[0] = fmaf(gu0, f.u0, M.m[0]);
  M.m[1] = fmaf(gu1, f.u1, M.m[1]);
  M.m[2] = fmaf(gu2, f.u2, M.m[2]);
  M.m[5] += gu0;
  M.m[6] += gu1;
  M.m[7] += gu2;
  M.m[8] = fmaf(gu0, gx, M.m[8]);
  M.m[9] = fmaf(gu0, gy, M.m[9]);
  M.m[10] = fmaf(gu0, gz, M.m[10]);
  M.m[11] = fmaf(gu1, gx, M.m[11]);
  M.m[12] = fmaf(gu1, gy, M.m[12]);
  M.m[13] = fmaf(gu1, gz, M.m[13]);
  M.m[14] = fmaf(gu2, gx, M.m[14]);
  M.m[15] = fmaf(gu2, gy, M.m[15]);
  M.m[16] = fmaf(gu2, gz, M.m[16]);
}
__device__ __forceinline__ void vox_bwd(const SQ& s, const Vox& f, float occ, float omo, float gocc,
                                        float sharp, float gx, float gy, float gz, Moments& M) {
  vox_bwd_lnG(s, f, gocc * (-sharp) * occ * omo * f.G, gx, gy, gz, M);  // dL/dln G
}

// the depths a ray is searched over (scan_render_kernel, free_space_kernel)
constexpr float kScanZLo = -3.f, kScanZHi = 4.f;  // a >= 0.05, t in [0, 1], |u| <= 1: z in [-sqrt 3, 1 + sqrt 3]

// log2 f at depth z and a value with the sign of df/dz.  A term with u_i = 0 is an exact 0: log2 = -inf, and
// lse2 is not asked for log2(0 + 0) (its max - min would be inf - inf)
__device__ __forceinline__ float scan_eval(const SQ& s, const RayU& r, float z, float& dsign) {
  const float u0 = fmaf(r.be[0], z, r.al[0]), u1 = fmaf(r.be[1], z, r.al[1]), u2 = fmaf(r.be[2], z, r.al[2]);
  const float lA = flog2(fabsf(u0)) * r.i2e2, lB = flog2(fabsf(u1)) * r.i2e2, lC = flog2(fabsf(u2)) * r.i2e1;
  float sA, sB, sE, sC;
  const bool noAB = fmaxf(lA, lB) == -INFINITY;
  const float l1 = lse2(lA, lB, &sA, &sB);
  const float lE = noAB ? -INFINITY : s.r21 * l1;
  const bool none = fmaxf(lE, lC) == -INFINITY;
  const float l2 = lse2(lE, lC, &sE, &sC);
  // d ln f / dz = (2 / e1) (sE (sA be0 / u0 + sB be1 / u1) + sC be2 / u2); a share of 0 over a u of 0 is 0
  constexpr float tiny = 1e-30f;
  const float g0 = (!noAB && fabsf(u0) > tiny) ? sA * r.be[0] * frcp(u0) : 0.f;
  const float g1 = (!noAB && fabsf(u1) > tiny) ? sB * r.be[1] * frcp(u1) : 0.f;
  const float g2 = (!none && fabsf(u2) > tiny) ? sC * r.be[2] * frcp(u2) : 0.f;
  dsign = none ? 0.f : fmaf(sE, g0 + g1, g2);
  return none ? -INFINITY : l2;
}

// 2^l - 1 without rounding 2^l first: points of a good fit lie on the surface, where F -> 1 and the
// energy is all cancellation.  |x| < 1/4: the exponential series to x^9 (next term < 1e-11 x).
__device__ __forceinline__ float exp2m1(float l) {
  const float x = l * kLn2;
  if (fabsf(x) >= 0.25f) return fexp2(l) - 1.f;
  float p = 1.f / 362880.f;
  p = fmaf(p, x, 1.f / 40320.f);
  p = fmaf(p, x, 1.f / 5040.f);
  p = fmaf(p, x, 1.f / 720.f);
  p = fmaf(p, x, 1.f / 120.f);
  p = fmaf(p, x, 1.f / 24.f);
  p = fmaf(p, x, 1.f / 6.f);
  p = fmaf(p, x, 0.5f);
  return fmaf(p * x, x, x);
}

}  // namespace sqr
