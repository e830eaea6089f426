// The classical fitting stack for gfx950 on the LeastSquares energy (classes.py:318-371): its normal equations on
// f64 MFMA, the Levenberg-Marquardt loop, the classical recovery's starts and selection around it
// (lsq_moments_kernel .. lsq_select_kernel), the free-space energy over every pixel's ray that the scored
// selection uses (free_space_kernel), and the one chain the recoveries run (recover_chain).  The points come from
// depth images (sqr_lsq_*, sqr_least_squares_normal_eq), from point lists (sqr_pts_*) or from the labelled parts of
// point lists (sqr_pts_labeled_*, sqr_pts_recover_parts with its assignment and seeding kernels): see "point sources".
#include "sqr_common.h"
#include "sqr_sq_dev.h"

#include <type_traits>

namespace sqr {

// -------------------------------------------------------------------------- LeastSquares normal equations
// Levenberg-Marquardt on the residuals r_k = sqrt(a0 a1 a2) (F(point_k) - 1) needs J^T J, J^T r and r^T r
// per sample, J_k = d r_k / d raw params.  With v = a0 a1 a2, r_k = sqrt(v) f_k (f_k = F - 1) and
// J_k = sqrt(v) j_k, j_k = dF/dparams + f_k / (2 a_i) on the three sizes, so all three products are v times
// the Gram matrix of the rows [j_k | f_k]: each thread forms its pixel's row in fp32 (vox_fwd, vox_bwd_lnG at
// dF/dln F = F, finalize_sample's chain applied per point), a wave lays its 64 rows out in LDS as a 64 x 16
// tile [j (12) | f | 0 0 0] and takes tile^T tile with 16 v_mfma_f64_16x16x4_f64 (A and B are the same
// register: lane l holds tile[4 s + (l >> 4)][l & 15] at step s; products of two floats are exact in
// float64, every sum is float64 in the instruction's fixed order).  A pixel that is not > 0 is a zero row.
// Waves are added in order per block, blocks in order per sample (lsq_normal_eq_finalize_kernel).
constexpr int kNeqT = 16;            // tile width: 12 Jacobian columns, the residual, 3 zero columns
constexpr int kNeqP = kNeqT * kNeqT;  // a block's partial: the whole 16 x 16 Gram matrix

// (dx, dy, dz) = point - t.  The rotation's partial derivatives use d_j = g_j - t_j directly instead of
// finalize_sample's (sum gu g_j) - (sum gu) t_j: per point there is nothing to cancel.
__device__ __forceinline__ void lsq_point_row(const SQ& s, float dx, float dy, float dz, float* row) {
  Vox f;
  vox_fwd(s, dx, dy, dz, f);
  const float fm1 = exp2m1(s.e1 * f.lF);
  Moments M;
  M.zero();
  vox_bwd_lnG(s, f, f.G, dx, dy, dz, M);
  float j[12];
#pragma unroll
  for (int i = 0; i < 3; ++i) j[i] = (0.5f * fm1 - M.m[i]) * s.ia[i];
  j[3] = M.m[3];
  j[4] = M.m[4];
  float sgv[3], gR[9];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    sgv[i] = M.m[5 + i] * s.ia[i];
#pragma unroll
    for (int k = 0; k < 3; ++k) gR[3 * i + k] = M.m[8 + 3 * i + k] * s.ia[i];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) j[5 + k] = -(s.M[k] * sgv[0] + s.M[3 + k] * sgv[1] + s.M[6 + k] * sgv[2]);
  // vjp of mat_from_quaternion at conj(q) = (x,y,z,w), as finalize_sample
  const float x = -s.q[0], y = -s.q[1], z = -s.q[2], w = s.q[3];
  const float qx = 2 * y * (gR[1] + gR[3]) + 2 * z * (gR[2] + gR[6]) + 2 * w * (gR[7] - gR[5]) - 4 * x * (gR[4] + gR[8]);
  const float qy = 2 * x * (gR[1] + gR[3]) + 2 * z * (gR[5] + gR[7]) + 2 * w * (gR[2] - gR[6]) - 4 * y * (gR[0] + gR[8]);
  const float qz = 2 * x * (gR[2] + gR[6]) + 2 * y * (gR[5] + gR[7]) + 2 * w * (gR[3] - gR[1]) - 4 * z * (gR[0] + gR[4]);
  const float qw = 2 * z * (gR[3] - gR[1]) + 2 * y * (gR[2] - gR[6]) + 2 * x * (gR[7] - gR[5]);
  j[8] = -qx;
  j[9] = -qy;
  j[10] = -qz;
  j[11] = qw;
#pragma unroll
  for (int i = 0; i < 12; ++i) row[i] = s.mask[i] != 0.f ? j[i] : 0.f;  // clamped: an exactly zero column
  row[12] = fm1;
  row[13] = row[14] = row[15] = 0.f;
}

// the point (c / R, 1 - r / R, z) of resized pixel `pix` of image b and whether it counts (z > 0: false for
// NaN); the resize arithmetic of least_squares_kernel
__device__ __forceinline__ bool lsq_point(const float* __restrict__ target, int b, int H, int W, int R, int pix,
                                          float& x, float& y, float& z) {
  x = y = z = 0.f;
  if (pix >= R * R) return false;
  const int r = pix / R, c = pix - r * R;
  const float sh = (float)H / (float)R, sw = (float)W / (float)R;
  const int sr = min((int)floorf((float)r * sh), H - 1);
  const int sc = min((int)floorf((float)c * sw), W - 1);
  z = target[((size_t)b * H + sr) * W + sc];
  x = (float)c / (float)R;
  y = 1.f - (float)r / (float)R;
  return z > 0.f;
}

// -------------------------------------------------------------------------- point sources
// Where the point-reading kernels (lsq_normal_eq_kernel, lsq_moments_kernel, lsq_extents_kernel) take slot i of
// sample b from: point(b, i, x, y, z) gives the fp32 point and whether it counts (a slot that does not is a zero
// row, a zero moment term, and ignored by min / max), slots() the slots per sample (one thread each, slot i =
// thread i mod 256 of block i / 256), nsrc() the images / clouds (sample s of a [K,nsrc] stack reads s mod nsrc).
// The kernels are templates on the source, so each source has its own straight-line code.
struct ImageSrc {  // the resized pixels of [Bimg,H,W] depth images in pixel order: lsq_point
  const float* target;
  int Bimg, H, W, R;
  __host__ __device__ int nsrc() const { return Bimg; }
  __host__ __device__ size_t slots() const { return (size_t)R * R; }
  __device__ __forceinline__ bool point(int b, int i, float& x, float& y, float& z) const {
    return lsq_point(target, b, H, W, R, i, x, y, z);
  }
};

// A point list: points [B,P,3] f32 (x, y, z), count [B] i32 (nullable: every cloud has P slots).  Slot i of cloud
// b counts iff i < count[b] (clamped into [0, P]) and all three coordinates are finite; no range is imposed on
// them (z <= 0 is an ordinary point).
struct ListSrc {
  const float* points;
  const int* count;
  int B, P;
  __host__ __device__ int nsrc() const { return B; }
  __host__ __device__ size_t slots() const { return (size_t)P; }
  __device__ __forceinline__ bool point(int b, int i, float& x, float& y, float& z) const {
    x = y = z = 0.f;
    const int n = count ? min(max(count[b], 0), P) : P;
    if (i >= n) return false;
    const float* p = points + ((size_t)b * P + i) * 3;
    const float px = p[0], py = p[1], pz = p[2];
    if (!(isfinite(px) && isfinite(py) && isfinite(pz))) return false;
    x = px;
    y = py;
    z = pz;
    return true;
  }
};

// The parts of labelled point lists: label [B,P] i32 beside a ListSrc's points and count.  Source v = b M + m is part
// m of cloud b: slot i of it is slot i of cloud b, and counts iff ListSrc counts it and label[b][i] == m.  Nothing
// is copied or compacted, so slot positions stay and with them the order of every sum: part (b, m) gives bitwise
// what the list gives for cloud b with every slot of another label set to NaN.  A label outside [0, M) belongs to
// no part.  The price: a part's launch walks all P slots of its cloud.
struct PartSrc {
  const float* points;
  const int* count;
  const int* label;
  int B, P, M;
  __host__ __device__ int nsrc() const { return B * M; }
  __host__ __device__ size_t slots() const { return (size_t)P; }
  __device__ __forceinline__ bool point(int v, int i, float& x, float& y, float& z) const {
    const int b = v / M, m = v - b * M;
    if (!ListSrc{points, count, B, P}.point(b, i, x, y, z)) return false;
    if (label[(size_t)b * P + i] == m) return true;
    x = y = z = 0.f;
    return false;
  }
};

// grid: (blocks_per_sample, S); one thread per slot of the source.  partials: [S][nblk][16][16] float64.  Sample b
// reads image / cloud b mod nsrc (the batched multi-start refinement's [K,nsrc] layout; nsrc = S: one each)
template <int NT, class Src>
__global__ void __launch_bounds__(NT) lsq_normal_eq_kernel(const float* __restrict__ params, const Src src,
                                                           double* __restrict__ partials) {
  static_assert(NT == kNeqP, "one thread per entry of the block's Gram matrix");
  typedef double d4 __attribute__((ext_vector_type(4)));
  __shared__ float4 tile[NT / 64][64 * kNeqT / 4];
  __shared__ double red[NT / 64][kNeqP];
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  SQ s;
  sq_load(params + 12 * b, s);
  float row[kNeqT];
#pragma unroll
  for (int i = 0; i < kNeqT; ++i) row[i] = 0.f;
  float gx, gy, z;
  if (src.point(b % src.nsrc(), blockIdx.x * NT + threadIdx.x, gx, gy, z))
    lsq_point_row(s, gx - s.t[0], gy - s.t[1], z - s.t[2], row);
#pragma unroll
  for (int i = 0; i < kNeqT / 4; ++i)
    tile[wid][lane * (kNeqT / 4) + i] = make_float4(row[4 * i], row[4 * i + 1], row[4 * i + 2], row[4 * i + 3]);
  __syncthreads();
  const float* tw = reinterpret_cast<const float*>(tile[wid]);
  d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int st = 0; st < 16; ++st) {
    const double v = (double)tw[(4 * st + (lane >> 4)) * kNeqT + (lane & 15)];
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(v, v, acc, 0, 0, 0);
  }
  // f64 C/D layout: register i of lane l is row (l >> 4) + 4 i, column l & 15
#pragma unroll
  for (int i = 0; i < 4; ++i) red[wid][((lane >> 4) + 4 * i) * kNeqT + (lane & 15)] = acc[i];
  __syncthreads();
  double sum = 0.0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) sum += red[w][threadIdx.x];
  partials[((size_t)b * gridDim.x + blockIdx.x) * kNeqP + threadIdx.x] = sum;
}

// grid: B blocks of 256 threads, thread (i, j) of a sample.  The blocks' partials in order, times a0 a1 a2;
// entry (i, j) of JtJ is read at (min, max), so the lower triangle is the upper one bitwise.
// e2 (nullable): a second copy of the energies.
__global__ void __launch_bounds__(kNeqP) lsq_normal_eq_finalize_kernel(const float* __restrict__ params,
                                                                       const double* __restrict__ partials, int nblk,
                                                                       double* __restrict__ JtJ,
                                                                       double* __restrict__ Jtr,
                                                                       double* __restrict__ energy,
                                                                       double* __restrict__ e2) {
  const int b = blockIdx.x;
  const int i = threadIdx.x / kNeqT, j = threadIdx.x % kNeqT;
  if (i > 12 || j > 12) return;
  const int src = min(i, j) * kNeqT + max(i, j);
  double acc = 0.0;
  for (int k = 0; k < nblk; ++k) acc += partials[((size_t)b * nblk + k) * kNeqP + src];
  const float* p = params + 12 * b;
  const double vol = (double)clampf(p[0], 0.05f, 1.f) * (double)clampf(p[1], 0.05f, 1.f) *
                     (double)clampf(p[2], 0.05f, 1.f);
  acc *= vol;
  if (i < 12 && j < 12) JtJ[(size_t)b * 144 + i * 12 + j] = acc;
  if (i == 12 && j < 12) Jtr[(size_t)b * 12 + j] = acc;
  if (i == 12 && j == 12) {
    energy[b] = acc;
    if (e2) e2[b] = acc;
  }
}

// -------------------------------------------------------------------------- Levenberg-Marquardt step
// clamp a, e, t into their ranges and divide q by its norm (kept as it is when the norm is 0 or not finite)
__device__ __forceinline__ void lm_project(const double* x, float* out) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    out[i] = clampf((float)x[i], 0.05f, 1.f);
    out[5 + i] = clampf((float)x[5 + i], 0.f, 1.f);
  }
  out[3] = clampf((float)x[3], 0.1f, 1.f);
  out[4] = clampf((float)x[4], 0.1f, 1.f);
  const double n = sqrt(x[8] * x[8] + x[9] * x[9] + x[10] * x[10] + x[11] * x[11]);
  const double inv = (n > 0.0 && isfinite(n)) ? 1.0 / n : 1.0;
#pragma unroll
  for (int i = 8; i < 12; ++i) out[i] = (float)(x[i] * inv);
}

__global__ void lm_init_kernel(const float* __restrict__ params_in, int B, double lambda0,
                               float* __restrict__ params, double* __restrict__ lambda,
                               int* __restrict__ accepted) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double x[12];
  float o[12];
  for (int i = 0; i < 12; ++i) x[i] = (double)params_in[12 * b + i];
  lm_project(x, o);
  for (int i = 0; i < 12; ++i) params[12 * b + i] = o[i];
  lambda[b] = lambda0;
  accepted[b] = 0;
}

constexpr double kLmLambdaMin = 1e-12, kLmLambdaMax = 1e12;
__device__ __forceinline__ double lm_clamp_lambda(double l) { return fmin(fmax(l, kLmLambdaMin), kLmLambdaMax); }

// one thread per sample, float64.  accept: the trial replaces the current state iff E_t < E (false for
// NaN), lambda *= down, else lambda *= up.  solve: (H + lambda diag H) delta = -g on the free set
// {i: H_ii > 0} as the Jacobi-scaled (S H S + lambda I) y = -S g, delta = S y, by Cholesky (an index off
// the free set is an identity row with a zero right side: y_i = 0 exactly); a pivot that is not a positive
// finite number, or a delta that is not finite, gives delta = 0 and lambda *= up.  The new trial
// parameters are lm_project(p + delta).
__global__ void __launch_bounds__(64) lm_step_kernel(int B, int accept, int solve, double up, double down,
                                                     float* __restrict__ p, double* __restrict__ Hc,
                                                     double* __restrict__ gc, double* __restrict__ Ec,
                                                     double* __restrict__ lambda, float* __restrict__ p_t,
                                                     const double* __restrict__ H_t, const double* __restrict__ g_t,
                                                     const double* __restrict__ E_t, double* __restrict__ delta,
                                                     int* __restrict__ accepted) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  p += 12 * (size_t)b;
  p_t += 12 * (size_t)b;
  Hc += 144 * (size_t)b;
  gc += 12 * (size_t)b;
  double lam = lambda[b];
  if (accept) {
    if (E_t[b] < Ec[b]) {
      for (int i = 0; i < 144; ++i) Hc[i] = H_t[144 * (size_t)b + i];
      for (int i = 0; i < 12; ++i) {
        gc[i] = g_t[12 * (size_t)b + i];
        p[i] = p_t[i];
      }
      Ec[b] = E_t[b];
      accepted[b] += 1;
      lam *= down;
    } else {
      lam *= up;
    }
    lam = lm_clamp_lambda(lam);
  }
  if (solve) {
    // every loop unrolled and no early exit, so sc, L and y stay in registers (indexed at run time they
    // live in scratch memory: 67 us per launch against 12 at B = 64); after a failed pivot the rest is
    // computed on NaNs and thrown away
    double sc[12], L[12][12], inv[12], y[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      const double d = Hc[13 * i];
      sc[i] = d > 0.0 ? 1.0 / sqrt(d) : 0.0;
    }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 12; ++j) {
#pragma unroll
      for (int i = j; i < 12; ++i) {
        double a;
        if (sc[i] == 0.0 || sc[j] == 0.0)
          a = i == j ? 1.0 : 0.0;
        else
          a = Hc[12 * j + i] * sc[i] * sc[j] + (i == j ? lam : 0.0);
#pragma unroll
        for (int k = 0; k < j; ++k) a -= L[i][k] * L[j][k];
        if (i == j) {
          ok = ok && a > 0.0 && isfinite(a);
          L[j][j] = sqrt(a);
          inv[j] = 1.0 / L[j][j];
        } else {
          L[i][j] = a * inv[j];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) {  // L z = -S g
      double a = sc[i] == 0.0 ? 0.0 : -sc[i] * gc[i];
#pragma unroll
      for (int k = 0; k < i; ++k) a -= L[i][k] * y[k];
      y[i] = a * inv[i];
    }
#pragma unroll
    for (int i = 11; i >= 0; --i) {  // L^T y = z
      double a = y[i];
#pragma unroll
      for (int k = i + 1; k < 12; ++k) a -= L[k][i] * y[k];
      y[i] = a * inv[i];
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      y[i] = sc[i] == 0.0 ? 0.0 : sc[i] * y[i];
      ok = ok && isfinite(y[i]);
    }
    if (!ok) {
#pragma unroll
      for (int i = 0; i < 12; ++i) y[i] = 0.0;
      lam = lm_clamp_lambda(lam * up);
    }
    double x[12];
    float o[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      delta[12 * (size_t)b + i] = y[i];
      x[i] = (double)p[i] + y[i];
    }
    lm_project(x, o);
#pragma unroll
    for (int i = 0; i < 12; ++i) p_t[i] = o[i];
  }
  lambda[b] = lam;
}

// -------------------------------------------------------------------------- LeastSquares starts (recovery)
// Solina & Bajcsy's start of the recovery, from the image's points alone (no counterpart in torch/): the
// centre of gravity and the principal axes of the points give position and orientation, the extents along
// those axes the sizes, an ellipsoid (e = e0) the shape; the three cyclic permutations of the axes are the
// three starts that sqr_lsq_recover refines.  Four launches, every one with least_squares_kernel's point
// rule: lsq_moments_kernel (n, sum p, sum p p^T per block), lsq_frame_kernel (centroid, covariance,
// eigen-frame per sample), lsq_extents_kernel (min / max of V^T p per block), lsq_starts_kernel (one thread
// per sample and start).  lsq_select_kernel picks the refined start of the lowest energy.
constexpr int kMomN = 10;         // upper triangle of the Gram matrix of the rows [x y z 1]: xx xy xz x yy yz y zz z n
constexpr int kJacobiSweeps = 8;  // cyclic Jacobi on a 3 x 3 converges quadratically: 4-5 sweeps reach an ulp

// grid: (blocks_per_sample, B); one thread per slot of the source.  partials: [B][nblk][kMomN] float64.  The
// products of two floats are exact in float64; lanes are summed by DPP (wave_sum_d), waves in order, as
// least_squares_kernel does, so the sums are bitwise defined.  A pixel that does not count is a zero row.
template <int NT, class Src>
__global__ void __launch_bounds__(NT) lsq_moments_kernel(const Src src, double* __restrict__ partials) {
  __shared__ double red[(NT / 64) * kMomN];
  const int b = blockIdx.y;
  float fx, fy, fz;
  const bool on = src.point(b, blockIdx.x * NT + threadIdx.x, fx, fy, fz);
  const double x = on ? (double)fx : 0.0, y = on ? (double)fy : 0.0, z = on ? (double)fz : 0.0;
  const double one = on ? 1.0 : 0.0;
  const double vals[kMomN] = {x * x, x * y, x * z, x, y * y, y * z, y, z * z, z, one};
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < kMomN; ++i) {
    const double v = wave_sum_d(vals[i]);
    if (lane == 0) red[wid * kMomN + i] = v;
  }
  __syncthreads();
  if (threadIdx.x < kMomN) {
    double acc = 0.0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) acc += red[w * kMomN + threadIdx.x];
    partials[((size_t)b * gridDim.x + blockIdx.x) * kMomN + threadIdx.x] = acc;
  }
}

// one Jacobi rotation of the symmetric 3 x 3 in the (p, q) plane, r the third index: a_pq -> 0, the
// eigenvector columns p and q of V rotated along (a proper rotation: det V stays +1)
__device__ __forceinline__ void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq,
                                              double& v0p, double& v0q, double& v1p, double& v1q, double& v2p,
                                              double& v2q) {
  const bool go = apq != 0.0;
  const double theta = (aqq - app) / (2.0 * (go ? apq : 1.0));
  // the smaller root of t^2 + 2 theta t - 1 = 0; theta^2 = inf gives t = 0
  double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  t = go ? t : 0.0;
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  app -= t * apq;
  aqq += t * apq;
  apq = go ? 0.0 : apq;
  const double rp = arp, rq = arq;
  arp = c * rp - s * rq;
  arq = s * rp + c * rq;
  const double a0 = v0p, b0 = v0q, a1 = v1p, b1 = v1q, a2 = v2p, b2 = v2q;
  v0p = c * a0 - s * b0; v0q = s * a0 + c * b0;
  v1p = c * a1 - s * b1; v1q = s * a1 + c * b1;
  v2p = c * a2 - s * b2; v2q = s * a2 + c * b2;
}

// the column (x, y, z) with its component of the largest magnitude (the first one on a tie) given the sign of
// `sign`
__device__ __forceinline__ void frame_sign(double& x, double& y, double& z, double sign) {
  const double ax = fabs(x), ay = fabs(y), az = fabs(z);
  const double lead = (ax >= ay && ax >= az) ? x : (ay >= az ? y : z);
  if (lead * sign < 0.0) {
    x = -x;
    y = -y;
    z = -z;
  }
}

// One thread per sample, float64: the blocks' moments in order, n, the centroid c = sum p / n, the covariance
// C = sum p p^T / n - c c^T and its eigen-decomposition by cyclic Jacobi, kJacobiSweeps sweeps over (0,1),
// (0,2), (1,2), fully unrolled on named scalars (registers; lm_step_kernel's lesson).  Eigenvalues ascending
// (a three-exchange sort, columns along); sign rule: the largest-magnitude component of column 0 is made
// negative and that of column 1 positive (frame_sign), column 2 = column 0 x column 1, so V is a proper rotation
// and a function of C alone.  (The four sign choices are the same body, but not the same Levenberg-Marquardt
// path: mat_from_quaternion is not normalised, so the Jacobian's radial part differs.  DESIGN.md has the four
// outcomes on the example images.)
// frame [B,3,3] row-major, the eigenvectors its columns.  No point: n = 0, zeros, V = I.
__global__ void __launch_bounds__(64) lsq_frame_kernel(const double* __restrict__ partials, int B, int nblk,
                                                       int* __restrict__ count, double* __restrict__ centroid,
                                                       double* __restrict__ eigenvalues,
                                                       double* __restrict__ frame) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double S[kMomN];
#pragma unroll
  for (int i = 0; i < kMomN; ++i) S[i] = 0.0;
  for (int k = 0; k < nblk; ++k) {
    const double* src = partials + ((size_t)b * nblk + k) * kMomN;
#pragma unroll
    for (int i = 0; i < kMomN; ++i) S[i] += src[i];
  }
  const double n = S[9];
  double cx = 0.0, cy = 0.0, cz = 0.0, l0 = 0.0, l1 = 0.0, l2 = 0.0;
  double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
  if (n > 0.0) {
    const double in = 1.0 / n;
    cx = S[3] * in;
    cy = S[6] * in;
    cz = S[8] * in;
    double a00 = S[0] * in - cx * cx, a01 = S[1] * in - cx * cy, a02 = S[2] * in - cx * cz;
    double a11 = S[4] * in - cy * cy, a12 = S[5] * in - cy * cz, a22 = S[7] * in - cz * cz;
#pragma unroll
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
      jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);  // (0,1), r = 2
      jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);  // (0,2), r = 1
      jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);  // (1,2), r = 0
    }
    l0 = a00;
    l1 = a11;
    l2 = a22;
    auto exch = [](double& la, double& lb, double& a0, double& b0, double& a1, double& b1, double& a2, double& b2) {
      if (la > lb) {
        double t;
        t = la; la = lb; lb = t;
        t = a0; a0 = b0; b0 = t;
        t = a1; a1 = b1; b1 = t;
        t = a2; a2 = b2; b2 = t;
      }
    };
    exch(l0, l1, v00, v01, v10, v11, v20, v21);
    exch(l1, l2, v01, v02, v11, v12, v21, v22);
    exch(l0, l1, v00, v01, v10, v11, v20, v21);
    frame_sign(v00, v10, v20, -1.0);
    frame_sign(v01, v11, v21, 1.0);
    v02 = v10 * v21 - v20 * v11;
    v12 = v20 * v01 - v00 * v21;
    v22 = v00 * v11 - v10 * v01;
  }
  count[b] = (int)n;
  centroid[3 * (size_t)b] = cx;
  centroid[3 * (size_t)b + 1] = cy;
  centroid[3 * (size_t)b + 2] = cz;
  eigenvalues[3 * (size_t)b] = l0;
  eigenvalues[3 * (size_t)b + 1] = l1;
  eigenvalues[3 * (size_t)b + 2] = l2;
  double* V = frame + 9 * (size_t)b;
  V[0] = v00; V[1] = v01; V[2] = v02;
  V[3] = v10; V[4] = v11; V[5] = v12;
  V[6] = v20; V[7] = v21; V[8] = v22;
}

// grid: (blocks_per_sample, B); one thread per slot of the source, float64.  partials: [B][nblk][6] = the block's
// minimum (0..2) and maximum (3..5) of V^T p along the three axes over its counted points (+inf / -inf where
// it has none).  min and max do not depend on the order: any reduction is bitwise reproducible.
template <int NT, class Src>
__global__ void __launch_bounds__(NT) lsq_extents_kernel(const Src src, const double* __restrict__ frame,
                                                         double* __restrict__ partials) {
  __shared__ double red[(NT / 64) * 6];
  const int b = blockIdx.y;
  const double* V = frame + 9 * (size_t)b;
  float fx, fy, fz;
  const bool on = src.point(b, blockIdx.x * NT + threadIdx.x, fx, fy, fz);
  double v[6];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double u = V[j] * (double)fx + V[3 + j] * (double)fy + V[6 + j] * (double)fz;
    v[j] = on ? u : (double)INFINITY;
    v[3 + j] = on ? u : -(double)INFINITY;
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    for (int o = 32; o >= 1; o >>= 1) {
      v[j] = fmin(v[j], __shfl_xor(v[j], o));
      v[3 + j] = fmax(v[3 + j], __shfl_xor(v[3 + j], o));
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < 6; ++j) red[wid * 6 + j] = v[j];
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    double acc = red[threadIdx.x];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w)
      acc = threadIdx.x < 3 ? fmin(acc, red[w * 6 + threadIdx.x]) : fmax(acc, red[w * 6 + threadIdx.x]);
    partials[((size_t)b * gridDim.x + blockIdx.x) * 6 + threadIdx.x] = acc;
  }
}

// One thread per (start k, sample b), float64, stored as float32 starts [3,B,12].  M_k = the columns
// (k, k+1, k+2 mod 3) of V: the local x, y, z axes in world coordinates, mat_from_quaternion(q) of the start
// (a cyclic permutation: det stays +1).  a = half the extents in that order, clamped into [0.05, 1];
// t = M_k (midpoint of the extents), clamped into [0, 1]; e = (e0, e0); q = the xyzw quaternion of M_k,
// taken from the largest of (trace, m00, m11, m22) (the first on a tie), so that the divisor s = 4 |largest
// component of q| >= 2.  No point, or a value that is not finite: a = 0.05, e = e0, t = 0.5, q = (0,0,0,1).
//
// nsets = 2 (sqr_lsq_starts6): starts [6,B,12], starts 3..5 are the depth-aware ones.  A depth image shows the
// front half of the body only, so the extent along the frame axis nearest the viewing direction is about half
// the true one and its midpoint too near the viewer (at +z).  ja = the column of V with the largest |V[2][ja]|
// (the first on a tie), ext = max - min along it; the hidden side is stretched by depth * ext: V[2][ja] > 0:
// min -= depth * ext, else max += depth * ext.  Everything after that is the same code with the same operands
// as starts 0..2, which take the stretch 0 * ext: x - 0 * ext = x exactly, so depth = 0 gives starts 0..2 again.
__global__ void __launch_bounds__(64) lsq_starts_kernel(int B, int nblk, int nsets, float e0, float depth,
                                                        const int* __restrict__ count,
                                                        const double* __restrict__ frame,
                                                        const double* __restrict__ extents,
                                                        float* __restrict__ starts) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 3 * nsets * B) return;
  const int kall = idx / B, b = idx - kall * B;
  const int k = kall % 3;
  const double stretch = kall >= 3 ? (double)depth : 0.0;
  float o[12] = {0.05f, 0.05f, 0.05f, e0, e0, 0.5f, 0.5f, 0.5f, 0.f, 0.f, 0.f, 1.f};
  if (count[b] > 0) {
    double M[9], half[3], mid[3];
    const double* V = frame + 9 * (size_t)b;
    const double z0 = fabs(V[6]), z1 = fabs(V[7]), z2 = fabs(V[8]);
    const int ja = (z0 >= z1 && z0 >= z2) ? 0 : (z1 >= z2 ? 1 : 2);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int ax = k + j >= 3 ? k + j - 3 : k + j;
      double lo = (double)INFINITY, hi = -(double)INFINITY;
      for (int blk = 0; blk < nblk; ++blk) {
        const double* src = extents + ((size_t)b * nblk + blk) * 6;
        lo = fmin(lo, src[ax]);
        hi = fmax(hi, src[3 + ax]);
      }
      if (ax == ja) {
        const double grow = stretch * (hi - lo);
        if (V[6 + ax] > 0.0) lo -= grow; else hi += grow;
      }
      half[j] = 0.5 * (hi - lo);
      mid[j] = 0.5 * (hi + lo);
#pragma unroll
      for (int i = 0; i < 3; ++i) M[3 * i + j] = frame[9 * (size_t)b + 3 * i + ax];
    }
    float c[12];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      c[i] = clampf((float)half[i], 0.05f, 1.f);
      c[5 + i] = clampf((float)(M[3 * i] * mid[0] + M[3 * i + 1] * mid[1] + M[3 * i + 2] * mid[2]), 0.f, 1.f);
    }
    c[3] = c[4] = e0;
    const double tr = M[0] + M[4] + M[8];
    double x, y, z, w;
    if (tr >= M[0] && tr >= M[4] && tr >= M[8]) {
      const double s = 2.0 * sqrt(1.0 + tr);
      w = 0.25 * s; x = (M[7] - M[5]) / s; y = (M[2] - M[6]) / s; z = (M[3] - M[1]) / s;
    } else if (M[0] >= M[4] && M[0] >= M[8]) {
      const double s = 2.0 * sqrt(1.0 + M[0] - M[4] - M[8]);
      x = 0.25 * s; y = (M[1] + M[3]) / s; z = (M[2] + M[6]) / s; w = (M[7] - M[5]) / s;
    } else if (M[4] >= M[8]) {
      const double s = 2.0 * sqrt(1.0 + M[4] - M[0] - M[8]);
      y = 0.25 * s; x = (M[1] + M[3]) / s; z = (M[5] + M[7]) / s; w = (M[2] - M[6]) / s;
    } else {
      const double s = 2.0 * sqrt(1.0 + M[8] - M[0] - M[4]);
      z = 0.25 * s; x = (M[2] + M[6]) / s; y = (M[5] + M[7]) / s; w = (M[3] - M[1]) / s;
    }
    c[8] = (float)x; c[9] = (float)y; c[10] = (float)z; c[11] = (float)w;
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 12; ++i) ok = ok && isfinite(c[i]);
    if (ok) {
#pragma unroll
      for (int i = 0; i < 12; ++i) o[i] = c[i];
    }
  }
  float* dst = starts + ((size_t)kall * B + b) * 12;
#pragma unroll
  for (int i = 0; i < 12; ++i) dst[i] = o[i];
}

// One thread per sample: the index of the lowest of the K energies [K,B] (the lowest k on a tie; NaN never
// wins; all NaN: 0), that start's parameters [K,B,12] and energy.
__global__ void __launch_bounds__(64) lsq_select_kernel(int B, int K, const float* __restrict__ params,
                                                        const double* __restrict__ energy,
                                                        float* __restrict__ out_params,
                                                        double* __restrict__ out_energy,
                                                        int* __restrict__ out_index) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int best = 0;
  double be = energy[b];
  for (int k = 1; k < K; ++k) {
    const double e = energy[(size_t)k * B + b];
    if (e < be || (be != be && e == e)) {
      best = k;
      be = e;
    }
  }
  const float* src = params + ((size_t)best * B + b) * 12;
  for (int i = 0; i < 12; ++i) out_params[12 * (size_t)b + i] = src[i];
  out_energy[b] = be;
  out_index[b] = best;
}

// -------------------------------------------------------------------------- free-space energy (selection)
// The point energy sees the image's points only: a model that sticks out where the image says "background",
// or in front of the visible surface, costs it nothing.  The free-space energy is summed over every resized
// pixel's ray (x, y) = (c / R, 1 - r / R), least_squares_kernel's pixel rule: along the segment [zlo, kScanZHi]
// of the ray, zlo = z + margin for a pixel z > 0 (nothing lies in front of the visible surface) and 0 for a
// pixel <= 0 (the scanner would have seen any surface there), the model must stay outside:
//   E_fs = a0 a1 a2 sum_pixels min(F(x, y, z*) - 1, 0)^2,  z* = argmin of F over the segment.
// A NaN pixel and an empty segment (zlo > kScanZHi) add nothing.  f = F^(1/e1) is convex in z (scan_render_kernel's
// note), so z* is where df/dz changes sign, clipped to the segment: a bisection with a fixed budget on
// scan_eval's sign, inside the slab |u_i| <= 1 cut with the segment; a ray whose segment misses the slab has
// F >= 1 there and adds an exact zero without a search (most background pixels).  The minimum is flat in z to
// second order, so the last bits of an interior z* do not matter (a z* at an end of the segment is that end
// exactly); the value is the point term's own F: vox_fwd, its zero fix and exp2m1.  A lane that has converged holds its bracket; the loop is left when no lane of the wave is live.
// grid: (blocks_per_sample, S); sample s reads image s mod Bimg.  partials: [S][nblk] float64 (a lane's term
// is fp32; lanes summed by DPP, waves in order, blocks in order in free_space_finalize_kernel).
constexpr int kFsIters = 26;  // a bracket at most 4 wide down to 6e-8

template <int NT>
__global__ void __launch_bounds__(NT) free_space_kernel(const float* __restrict__ params,
                                                        const float* __restrict__ target, int Bimg, int H, int W,
                                                        int R, float margin, double* __restrict__ partials) {
  __shared__ double red[NT / 64];
  const int b = blockIdx.y;
  SQ s;
  sq_load(params + 12 * (size_t)b, s);
  const int pix = blockIdx.x * NT + threadIdx.x;
  bool hit = false;
  float gx = 0.f, gy = 0.f, z0 = 0.f, z1 = 0.f;
  RayU ru;
  if (pix < R * R) {
    const int r = pix / R, c = pix - r * R;
    const float sh = (float)H / (float)R, sw = (float)W / (float)R;
    const int sr = min((int)floorf((float)r * sh), H - 1);
    const int sc = min((int)floorf((float)c * sw), W - 1);
    const float z = target[((size_t)(b % Bimg) * H + sr) * W + sc];
    gx = (float)c / (float)R;
    gy = 1.f - (float)r / (float)R;
    z0 = z > 0.f ? z + margin : 0.f;
    z1 = kScanZHi;
    hit = z == z && z0 <= z1;
  }
  ray_u(s, gx - s.t[0], gy - s.t[1], ru);
#pragma unroll
  for (int i = 0; i < 3; ++i) {  // the slab, as scan_render_kernel
    const bool flat = ru.be[i] == 0.f;
    const float ib = 1.f / (flat ? 1.f : ru.be[i]);
    const float za = (-1.f - ru.al[i]) * ib, zb = (1.f - ru.al[i]) * ib;
    hit = hit && !(flat && fabsf(ru.al[i]) > 1.f);
    z0 = flat ? z0 : fmaxf(z0, fminf(za, zb));
    z1 = flat ? z1 : fminf(z1, fmaxf(za, zb));
  }
  hit = hit && z0 <= z1;
  float term = 0.f;
  if (__any(hit)) {
    float lo = z0, hi = z1;
    bool live = hit;
    for (int it = 0; it < kFsIters; ++it) {
      if (!__any(live)) break;
      const float mid = 0.5f * (lo + hi);
      float d;
      scan_eval(s, ru, mid, d);
      live = live && mid > lo && mid < hi;
      if (live) {
        if (d > 0.f) hi = mid; else lo = mid;  // f rises: the minimum lies below
      }
    }
    if (hit) {
      // an end of the bracket that never moved is the minimiser itself: the minimum of a segment that starts
      // behind it lies at the start exactly, where F is not flat (half a last bracket off is a one-sided error)
      const float zs = lo == z0 ? z0 : (hi == z1 ? z1 : 0.5f * (lo + hi));
      Vox f;
      vox_fwd(s, gx - s.t[0], gy - s.t[1], zs - s.t[2], f);
      const float fm1 = fminf(exp2m1(s.e1 * f.lF), 0.f);
      term = fm1 * fm1;
    }
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const double v = wave_sum_d((double)term);
  if (lane == 0) red[wid] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double acc = 0.0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) acc += red[w];
    partials[(size_t)b * gridDim.x + blockIdx.x] = acc;
  }
}

// One thread per sample: E_fs = a0 a1 a2 * (the blocks' partials in order).  score (nullable) = energy + w E_fs,
// the multi-start recovery's selection score; w = 0: the energy itself, bitwise, whatever E_fs is.
__global__ void __launch_bounds__(64) free_space_finalize_kernel(const float* __restrict__ params,
                                                                 const double* __restrict__ partials, int S, int nblk,
                                                                 double* __restrict__ energy_fs,
                                                                 const double* __restrict__ energy, double w,
                                                                 double* __restrict__ score) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= S) return;
  double acc = 0.0;
  for (int k = 0; k < nblk; ++k) acc += partials[(size_t)b * nblk + k];
  const float* p = params + 12 * (size_t)b;
  const double vol = (double)clampf(p[0], 0.05f, 1.f) * (double)clampf(p[1], 0.05f, 1.f) *
                     (double)clampf(p[2], 0.05f, 1.f);
  const double fs = vol * acc;
  energy_fs[b] = fs;
  if (score) score[b] = w == 0.0 ? energy[b] : energy[b] + w * fs;
}

// extra starts [n] floats copied behind the computed ones (a launch, so the chain stays a chain of kernels)
__global__ void lsq_copy_kernel(const float* __restrict__ src, long long n, float* __restrict__ dst) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

// the winner's point energy and free-space energy: row index[b] of [K,B]
__global__ void __launch_bounds__(64) lsq_gather_kernel(int B, const int* __restrict__ index,
                                                        const double* __restrict__ energy,
                                                        const double* __restrict__ energy_fs,
                                                        double* __restrict__ out_energy,
                                                        double* __restrict__ out_fs) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const size_t at = (size_t)index[b] * B + b;
  out_energy[b] = energy[at];
  out_fs[b] = energy_fs[at];
}

// -------------------------------------------------------------------------- several parts: assign and seed
// A cloud of several bodies is fitted by alternating "which part explains this point" (pts_assign_kernel) with
// "refit every part" (the chains above on a PartSrc).  The assignment's metric is Solina's radial Euclidean distance
//   d = |p - t| |1 - f^(-1/2)|,  f = F^e1 (f - 1 is lsq_point_row's row[12]: vox_fwd, its clamps and zero fix),
// the distance along the ray from the part's centre to where that ray meets the surface: exact for a sphere and in
// the cloud's units, so a small part is not favoured as the volume-weighted residual would favour it.
// 1 - f^(-1/2) = -(2^(-e1 lF / 2) - 1) is taken with exp2m1: points of a good fit lie where it is all cancellation.
// A d that is not finite counts as +inf.  The seeding's metric (kCentre) is the squared distance to a centre,
// (dx dx + dy dy) + dz dz with every operation rounded (no contraction: the host reference repeats it bit for bit).
constexpr int kMaxParts = 16;
constexpr int kPartRow = 20;  // a part's row in LDS: ia 3, t 3, M 9, e1, ie1, ie2, r21, NaN flag (radial) or the centre's 3

__device__ __forceinline__ float sqdist_rn(float px, float py, float pz, float cx, float cy, float cz) {
#pragma clang fp contract(off)
  const float dx = px - cx, dy = py - cy, dz = pz - cz;
  const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
  const float xy = xx + yy;
  return xy + zz;
}

// grid: (blocks_per_cloud, B); one thread per slot, the slot-to-thread map of the kernels above.  rows: the cloud's M
// parameter rows [B,M,12] (or centres [B,M,3], kCentre), the same for the whole block: threads 0 .. M-1 prepare one
// each (sq_load) and leave what the loop needs in LDS.  label [B,P] i32 = argmin_m d (a later m must be strictly
// nearer: the lowest m on a tie, 0 when every d is +inf), -1 for a slot that does not count (ListSrc's rule); dist
// [B,P] f32 the winning d, 0 where the label is -1.  prev (nullable): the labels before; a counting slot whose label
// differs from it is counted.  Per block, in order (lanes by DPP or ballot, waves in order):
//   pdist [B][nblk][M] f64 the sum of dist per part, pcount [B][nblk][M] i32, pchanged [B][nblk] i32
template <int NT, bool kCentre>
__global__ void __launch_bounds__(NT) pts_assign_kernel(const float* __restrict__ points, const int* __restrict__ count,
                                                        int B, int P, int M, const float* __restrict__ rows,
                                                        const int* __restrict__ prev, int* __restrict__ label,
                                                        float* __restrict__ dist, double* __restrict__ pdist,
                                                        int* __restrict__ pcount, int* __restrict__ pchanged) {
  __shared__ float part[kMaxParts][kPartRow];
  __shared__ double red_d[NT / 64][kMaxParts];
  __shared__ int red_n[NT / 64][kMaxParts + 1];
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if ((int)threadIdx.x < M) {
    float* r = part[threadIdx.x];
    if constexpr (kCentre) {
      const float* c = rows + ((size_t)b * M + threadIdx.x) * 3;
      r[0] = c[0];
      r[1] = c[1];
      r[2] = c[2];
    } else {
      SQ s;
      sq_load(rows + ((size_t)b * M + threadIdx.x) * 12, s);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        r[i] = s.ia[i];
        r[3 + i] = s.t[i];
      }
#pragma unroll
      for (int i = 0; i < 9; ++i) r[6 + i] = s.M[i];
      r[15] = s.e1;
      r[16] = s.ie1;
      r[17] = s.ie2;
      r[18] = s.r21;
      // vox_fwd's fmaxf(., FLT_MIN) drops a NaN square, so a NaN size or rotation would still give a finite d
      // (the host reference's NaN goes through to d): a row with a NaN parameter has no distance
      const float* raw = rows + ((size_t)b * M + threadIdx.x) * 12;
      bool nan = false;
#pragma unroll
      for (int i = 0; i < 12; ++i) nan = nan || raw[i] != raw[i];
      r[19] = nan ? 1.f : 0.f;
    }
  }
  __syncthreads();
  const int i = blockIdx.x * NT + threadIdx.x;
  float x, y, z;
  const bool on = ListSrc{points, count, B, P}.point(b, i, x, y, z);
  int best = 0;
  float bd = INFINITY;
  for (int m = 0; m < M; ++m) {
    const float* r = part[m];
    float d;
    if constexpr (kCentre) {
      d = sqdist_rn(x, y, z, r[0], r[1], r[2]);
    } else {
      SQ s;  // the fields vox_fwd reads
#pragma unroll
      for (int k = 0; k < 3; ++k) s.ia[k] = r[k];
#pragma unroll
      for (int k = 0; k < 9; ++k) s.M[k] = r[6 + k];
      s.e1 = r[15];
      s.ie1 = r[16];
      s.ie2 = r[17];
      s.r21 = r[18];
      const float dx = x - r[3], dy = y - r[4], dz = z - r[5];
      Vox f;
      vox_fwd(s, dx, dy, dz, f);
      d = sqrtf(fmaf(dx, dx, fmaf(dy, dy, dz * dz))) * fabsf(exp2m1(-0.5f * s.e1 * f.lF));
      if (r[19] != 0.f) d = INFINITY;
    }
    d = d < INFINITY ? d : INFINITY;  // NaN too
    if (m == 0 || d < bd) {
      bd = d;
      best = m;
    }
  }
  const int lab = on ? best : -1;
  const float dw = on ? bd : 0.f;
  bool moved = false;
  if (i < P) {
    const size_t at = (size_t)b * P + i;
    label[at] = lab;
    if (dist) dist[at] = dw;
    moved = prev && on && prev[at] != lab;
  }
  for (int m = 0; m < M; ++m) {  // every lane is active here: wave_sum_d's condition
    const bool mine = lab == m;
    const double v = wave_sum_d(mine ? (double)dw : 0.0);
    const int n = __popcll(__ballot(mine));
    if (lane == 0) {
      red_d[wid][m] = v;
      red_n[wid][m] = n;
    }
  }
  const int nmoved = __popcll(__ballot(moved));
  if (lane == 0) red_n[wid][kMaxParts] = nmoved;
  __syncthreads();
  const size_t blk = (size_t)b * gridDim.x + blockIdx.x;
  if ((int)threadIdx.x < M) {
    double v = 0.0;
    int n = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
      v += red_d[w][threadIdx.x];
      n += red_n[w][threadIdx.x];
    }
    pdist[blk * M + threadIdx.x] = v;
    pcount[blk * M + threadIdx.x] = n;
  }
  if (threadIdx.x == 0) {
    int n = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) n += red_n[w][kMaxParts];
    pchanged[blk] = n;
  }
}

// One thread per part (b, m): the blocks' partials in order.  changed (nullable) [B]: written by the thread of m = 0.
__global__ void __launch_bounds__(64) pts_assign_finalize_kernel(int B, int M, int nblk,
                                                                 const double* __restrict__ pdist,
                                                                 const int* __restrict__ pcount,
                                                                 const int* __restrict__ pchanged,
                                                                 int* __restrict__ part_count,
                                                                 double* __restrict__ part_dist,
                                                                 int* __restrict__ changed) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= B * M) return;
  const int b = v / M, m = v - b * M;
  double d = 0.0;
  int n = 0;
  for (int k = 0; k < nblk; ++k) {
    d += pdist[((size_t)b * nblk + k) * M + m];
    n += pcount[((size_t)b * nblk + k) * M + m];
  }
  part_dist[v] = d;
  part_count[v] = n;
  if (m == 0 && changed) {
    int c = 0;
    for (int k = 0; k < nblk; ++k) c += pchanged[(size_t)b * nblk + k];
    changed[b] = c;
  }
}

// the farther of two (distance, slot) candidates, the lower slot at equal distance
__device__ __forceinline__ void far_take(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) {
    v = ov;
    i = oi;
  }
}

// Farthest-point seeding, one block per cloud, M passes over its slots (thread t owns the slots t mod NT, so the
// running minimum mind [B,P] f32 needs no barrier).  Pass 0 measures from the first counting slot and its farthest
// slot is seed 0; pass k >= 1 folds seed k-1 into mind (pass 1 sets it) and the slot of the largest mind is seed k.
// A candidate must be strictly farther than the running best, which starts at (distance 0, the slot measured
// from): the lowest slot wins a tie, and a cloud that has run out of distinct points repeats its last seed.
// seeds [B,M] i32, centres [B,M,3] f32 = the seeds' points.  No counting slot: seeds -1, centres 0.
template <int NT>
__global__ void __launch_bounds__(NT) pts_fps_kernel(const float* __restrict__ points, const int* __restrict__ count,
                                                     int B, int P, int M, float* __restrict__ mind,
                                                     int* __restrict__ seeds, float* __restrict__ centres) {
  __shared__ float rv[2][NT / 64];
  __shared__ int ri[2][NT / 64];
  __shared__ int seed_of[kMaxParts];
  const int b = blockIdx.x;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const ListSrc src{points, count, B, P};
  float x, y, z;
  int first = P;
  for (int i = threadIdx.x; i < P && first == P; i += NT)
    if (src.point(b, i, x, y, z)) first = i;
  for (int o = 32; o >= 1; o >>= 1) first = min(first, __shfl_xor(first, o));
  if (lane == 0) ri[1][wid] = first;
  __syncthreads();
  first = ri[1][0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w) first = min(first, ri[1][w]);
  if (first == P) {  // the same in every thread
    if ((int)threadIdx.x < M) {
      seeds[(size_t)b * M + threadIdx.x] = -1;
      float* c = centres + ((size_t)b * M + threadIdx.x) * 3;
      c[0] = c[1] = c[2] = 0.f;
    }
    return;
  }
  float* md = mind + (size_t)b * P;
  int from = first;
  for (int k = 0; k < M; ++k) {
    // pass k writes buffer k & 1; a wave reaches pass k + 2's write only through pass k + 1's barrier, behind
    // every wave's reads of pass k
    const float* c = points + ((size_t)b * P + from) * 3;
    const float cx = c[0], cy = c[1], cz = c[2];
    float bv = 0.f;
    int bi = from;
    for (int i = threadIdx.x; i < P; i += NT) {
      if (!src.point(b, i, x, y, z)) continue;
      float d = sqdist_rn(x, y, z, cx, cy, cz);
      if (k == 1) md[i] = d;
      if (k > 1) {
        d = fminf(md[i], d);
        md[i] = d;
      }
      if (d > bv) {  // ascending slots: the first of equal distances stays
        bv = d;
        bi = i;
      }
    }
    for (int o = 32; o >= 1; o >>= 1) far_take(bv, bi, __shfl_xor(bv, o), __shfl_xor(bi, o));
    if (lane == 0) {
      rv[k & 1][wid] = bv;
      ri[k & 1][wid] = bi;
    }
    __syncthreads();
    bv = rv[k & 1][0];
    bi = ri[k & 1][0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) far_take(bv, bi, rv[k & 1][w], ri[k & 1][w]);
    from = bi;
    if (threadIdx.x == 0) seed_of[k] = bi;
  }
  __syncthreads();
  if ((int)threadIdx.x < M) {
    const int s = seed_of[threadIdx.x];
    seeds[(size_t)b * M + threadIdx.x] = s;
    const float* p = points + ((size_t)b * P + s) * 3;
    float* c = centres + ((size_t)b * M + threadIdx.x) * 3;
    c[0] = p[0];
    c[1] = p[1];
    c[2] = p[2];
  }
}

// One thread per part (b, m): its centre := the mean of its counting points, from lsq_moments_kernel's partials on
// the PartSrc ([B M][nblk][kMomN]: sum x = 3, sum y = 6, sum z = 8, n = 9), blocks in order, float64, rounded to
// float32 once.  An empty part keeps its centre.
__global__ void __launch_bounds__(64) pts_centre_kernel(int BM, int nblk, const double* __restrict__ partials,
                                                        float* __restrict__ centres) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= BM) return;
  double sx = 0.0, sy = 0.0, sz = 0.0, n = 0.0;
  for (int k = 0; k < nblk; ++k) {
    const double* src = partials + ((size_t)v * nblk + k) * kMomN;
    sx += src[3];
    sy += src[6];
    sz += src[8];
    n += src[9];
  }
  if (n > 0.0) {
    centres[3 * (size_t)v] = (float)(sx / n);
    centres[3 * (size_t)v + 1] = (float)(sy / n);
    centres[3 * (size_t)v + 2] = (float)(sz / n);
  }
}

}  // namespace sqr

using namespace sqr;

// ============================================================================ C ABI
// Blocks of 256 slots per sample: the grid of every launch over a source (kNeqP = 256 too).  The byte counts below
// are written on the slots per sample, R^2 for images and P for point lists, so that both sources share them.
static_assert(kNeqP == 256, "the normal equations and the starts share one block count");
static size_t slot_blocks(size_t slots) { return (slots + 255) / 256; }
static size_t image_slots(int R) { return (size_t)R * R; }
constexpr int kMaxListSlots = 1 << 20;  // P of a point list: the slots of R = 1024

static size_t normal_eq_bytes(size_t S, size_t slots) { return S * slot_blocks(slots) * kNeqP * sizeof(double); }

extern "C" size_t sqr_least_squares_normal_eq_workspace_bytes(int B, int R) {
  if (B <= 0 || R <= 0) return 0;
  return normal_eq_bytes((size_t)B, image_slots(R));
}

extern "C" size_t sqr_pts_normal_eq_workspace_bytes(int S, int P) {
  if (S <= 0 || P <= 0) return 0;
  return normal_eq_bytes((size_t)S, (size_t)P);
}

// What an entry checks of its source before anything else, `who` the entry's name in the messages
static int check_source(const char* who, const ImageSrc& src) {
  SQR_CHECK_ARG(src.R >= 1 && src.R <= 1024, "%s: R=%d out of range [1,1024]", who, src.R);
  SQR_CHECK_ARG(src.H >= 1 && src.W >= 1, "%s: bad target size %dx%d", who, src.H, src.W);
  SQR_CHECK_ARG(src.target, "%s: null pointer", who);
  return SQR_OK;
}

static int check_source(const char* who, const ListSrc& src) {
  SQR_CHECK_ARG(src.P >= 1 && src.P <= kMaxListSlots, "%s: P=%d out of range [1,%d]", who, src.P, kMaxListSlots);
  SQR_CHECK_ARG(src.points, "%s: null pointer", who);
  return SQR_OK;
}

static int check_source(const char* who, const PartSrc& src) {
  SQR_CHECK_ARG(src.M >= 1 && src.M <= kMaxParts, "%s: M=%d out of range [1,%d]", who, src.M, kMaxParts);
  SQR_CHECK_ARG(src.P >= 1 && src.P <= kMaxListSlots, "%s: P=%d out of range [1,%d]", who, src.P, kMaxListSlots);
  SQR_CHECK_ARG(src.points && src.label, "%s: null pointer", who);
  return SQR_OK;
}

// the two launches of the normal equations over B samples (arguments checked by the callers)
template <class Src>
static int launch_normal_eq(hipStream_t st, const float* params, const Src& src, int B, double* JtJ, double* Jtr,
                            double* energy, double* energy_copy, double* partials) {
  const int nblk = (int)slot_blocks(src.slots());
  hipLaunchKernelGGL((lsq_normal_eq_kernel<kNeqP, Src>), dim3(nblk, B), dim3(kNeqP), 0, st, params, src, partials);
  SQR_HIP_LAUNCH_CHECK("lsq_normal_eq_kernel");
  hipLaunchKernelGGL(lsq_normal_eq_finalize_kernel, dim3(B), dim3(kNeqP), 0, st, params, partials, nblk, JtJ, Jtr,
                     energy, energy_copy);
  SQR_HIP_LAUNCH_CHECK("lsq_normal_eq_finalize_kernel");
  return SQR_OK;
}

extern "C" int sqr_least_squares_normal_eq(const float* params, const float* target, int B, int H, int W, int R,
                                           double* JtJ, double* Jtr, double* energy, void* workspace,
                                           size_t workspace_bytes, void* stream) {
  SQR_CHECK_ARG(B >= 1 && B <= 65535, "least_squares_normal_eq: B=%d out of range [1,65535]", B);
  SQR_CHECK_ARG(R >= 1 && R <= 1024, "least_squares_normal_eq: R=%d out of range [1,1024]", R);
  SQR_CHECK_ARG(H >= 1 && W >= 1, "least_squares_normal_eq: bad target size %dx%d", H, W);
  SQR_CHECK_ARG(params && target && JtJ && Jtr && energy && workspace, "least_squares_normal_eq: null pointer");
  const size_t need = sqr_least_squares_normal_eq_workspace_bytes(B, R);
  if (workspace_bytes < need) {
    set_error("least_squares_normal_eq: workspace %zu < %zu bytes", workspace_bytes, need);
    return SQR_E_WORKSPACE;
  }
  return launch_normal_eq(as_stream(stream), params, ImageSrc{target, B, H, W, R}, B, JtJ, Jtr, energy, nullptr,
                          (double*)workspace);
}

extern "C" int sqr_pts_normal_eq(const float* params, const float* points, const int* count, int S, int B, int P,
                                 double* JtJ, double* Jtr, double* energy, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  SQR_CHECK_ARG(B >= 1 && S >= B && S <= 65535 && S % B == 0,
                "pts_normal_eq: S=%d must be a multiple of B=%d in [B,65535]", S, B);
  const ListSrc src{points, count, B, P};
  const int rc = check_source("pts_normal_eq", src);
  if (rc != SQR_OK) return rc;
  SQR_CHECK_ARG(params && JtJ && Jtr && energy && workspace, "pts_normal_eq: null pointer");
  const size_t need = sqr_pts_normal_eq_workspace_bytes(S, P);
  SQR_CHECK_ARG(workspace_bytes >= need, "pts_normal_eq: workspace %zu < %zu bytes", workspace_bytes, need);
  return launch_normal_eq(as_stream(stream), params, src, S, JtJ, Jtr, energy, nullptr, (double*)workspace);
}

extern "C" int sqr_lsq_lm_step(int B, int accept, int solve, double up, double down, float* params, double* JtJ,
                               double* Jtr, double* energy, double* lambda, float* params_trial,
                               const double* JtJ_trial, const double* Jtr_trial, const double* energy_trial,
                               double* delta, int* accepted, void* stream) {
  SQR_CHECK_ARG(B >= 1, "lsq_lm_step: B=%d must be >= 1", B);
  SQR_CHECK_ARG(up > 1.0, "lsq_lm_step: up=%g must be > 1", up);
  SQR_CHECK_ARG(down > 0.0 && down < 1.0, "lsq_lm_step: down=%g outside (0,1)", down);
  SQR_CHECK_ARG(params && JtJ && Jtr && energy && lambda, "lsq_lm_step: null state pointer");
  SQR_CHECK_ARG(!accept || (params_trial && JtJ_trial && Jtr_trial && energy_trial && accepted),
                "lsq_lm_step: accept without a trial state");
  SQR_CHECK_ARG(!solve || (params_trial && delta), "lsq_lm_step: solve without params_trial / delta");
  hipLaunchKernelGGL(lm_step_kernel, dim3((B + 63) / 64), dim3(64), 0, as_stream(stream), B, accept, solve, up, down,
                     params, JtJ, Jtr, energy, lambda, params_trial, JtJ_trial, Jtr_trial, energy_trial, delta,
                     accepted);
  SQR_HIP_LAUNCH_CHECK("lm_step_kernel");
  return SQR_OK;
}

// float64 first, then the trial parameters: [JtJ 144][Jtr 12][lambda 1][JtJ_t 144][Jtr_t 12][E_t 1][delta 12]
// per sample, the normal equations' partials, params_trial [B,12] f32
constexpr size_t kLmDoubles = 144 + 12 + 1 + 144 + 12 + 1 + 12;

static size_t lm_refine_bytes(size_t S, size_t slots) {
  return S * kLmDoubles * sizeof(double) + normal_eq_bytes(S, slots) + S * 12 * sizeof(float);
}

extern "C" size_t sqr_lsq_lm_refine_workspace_bytes(int B, int R) {
  if (B <= 0 || R <= 0) return 0;
  return lm_refine_bytes((size_t)B, image_slots(R));
}

extern "C" size_t sqr_pts_lm_refine_workspace_bytes(int S, int P) {
  if (S <= 0 || P <= 0) return 0;
  return lm_refine_bytes((size_t)S, (size_t)P);
}

// The chain of sqr_lsq_lm_refine over B samples, sample b on image / cloud b mod src.nsrc() (arguments checked by
// the callers; the workspace is lm_refine_bytes(B, src.slots())).  Every sample is on its own and every sum has a
// fixed order, so a sample's result does not depend on B.
template <class Src>
static int lm_refine_chain(const float* params_in, const Src& src, int B, int iters, double lambda0, double up,
                           double down, float* params_out, double* energy_before, double* energy_after,
                           int* accepted, void* workspace, void* stream) {
  hipStream_t st = as_stream(stream);
  const size_t nb = (size_t)B;
  double* JtJ = (double*)workspace;
  double* Jtr = JtJ + 144 * nb;
  double* lambda = Jtr + 12 * nb;
  double* JtJ_t = lambda + nb;
  double* Jtr_t = JtJ_t + 144 * nb;
  double* E_t = Jtr_t + 12 * nb;
  double* delta = E_t + nb;
  double* partials = delta + 12 * nb;
  float* p_t = (float*)(partials + nb * slot_blocks(src.slots()) * kNeqP);
  hipLaunchKernelGGL(lm_init_kernel, dim3((B + 63) / 64), dim3(64), 0, st, params_in, B, lambda0, params_out, lambda,
                     accepted);
  SQR_HIP_LAUNCH_CHECK("lm_init_kernel");
  int rc = launch_normal_eq(st, params_out, src, B, JtJ, Jtr, energy_after, energy_before, partials);
  if (rc != SQR_OK) return rc;
  for (int it = 0; it <= iters && iters > 0; ++it) {
    // round it: accept the trial of the round before (none in round 0), solve for the next one and
    // evaluate it; the last pass only accepts
    const int accept = it > 0, solve = it < iters;
    rc = sqr_lsq_lm_step(B, accept, solve, up, down, params_out, JtJ, Jtr, energy_after, lambda, p_t, JtJ_t, Jtr_t,
                         E_t, delta, accepted, stream);
    if (rc != SQR_OK) return rc;
    if (solve) {
      rc = launch_normal_eq(st, p_t, src, B, JtJ_t, Jtr_t, E_t, nullptr, partials);
      if (rc != SQR_OK) return rc;
    }
  }
  return SQR_OK;
}

// The refinement entries behind their own batch bound, `who` the entry's name in the messages: K slices of B
// samples in one chain (sqr_lsq_lm_refine: K = 1)
template <class Src>
static int lm_refine_entry(const char* who, const float* params_in, const Src& src, int K, int B, int iters,
                           double lambda0, double up, double down, float* params_out, double* energy_before,
                           double* energy_after, int* accepted, void* workspace, size_t workspace_bytes,
                           void* stream) {
  const int rc = check_source(who, src);
  if (rc != SQR_OK) return rc;
  SQR_CHECK_ARG(iters >= 0, "%s: iters=%d must be >= 0", who, iters);
  SQR_CHECK_ARG(lambda0 > 0.0, "%s: lambda0=%g must be > 0", who, lambda0);
  SQR_CHECK_ARG(up > 1.0, "%s: up=%g must be > 1", who, up);
  SQR_CHECK_ARG(down > 0.0 && down < 1.0, "%s: down=%g outside (0,1)", who, down);
  SQR_CHECK_ARG(params_in && params_out && energy_before && energy_after && accepted && workspace,
                "%s: null pointer", who);
  const size_t need = lm_refine_bytes((size_t)K * B, src.slots());
  SQR_CHECK_ARG(workspace_bytes >= need, "%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
  return lm_refine_chain(params_in, src, K * B, iters, lambda0, up, down, params_out, energy_before, energy_after,
                         accepted, workspace, stream);
}

extern "C" int sqr_lsq_lm_refine(const float* params_in, const float* target, int B, int H, int W, int R, int iters,
                                 double lambda0, double up, double down, float* params_out, double* energy_before,
                                 double* energy_after, int* accepted, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  SQR_CHECK_ARG(B >= 1 && B <= 65535, "lsq_lm_refine: B=%d out of range [1,65535]", B);
  return lm_refine_entry("lsq_lm_refine", params_in, ImageSrc{target, B, H, W, R}, 1, B, iters, lambda0, up, down,
                         params_out, energy_before, energy_after, accepted, workspace, workspace_bytes, stream);
}

extern "C" int sqr_lsq_lm_refine_multi(const float* params_in, const float* target, int K, int B, int H, int W, int R,
                                       int iters, double lambda0, double up, double down, float* params_out,
                                       double* energy_before, double* energy_after, int* accepted, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  SQR_CHECK_ARG(K >= 1 && B >= 1 && (long long)K * B <= 65535, "lsq_lm_refine_multi: K=%d x B=%d out of range [1,65535]",
                K, B);
  return lm_refine_entry("lsq_lm_refine_multi", params_in, ImageSrc{target, B, H, W, R}, K, B, iters, lambda0, up,
                         down, params_out, energy_before, energy_after, accepted, workspace, workspace_bytes, stream);
}

extern "C" int sqr_pts_lm_refine(const float* params_in, const float* points, const int* count, int K, int B, int P,
                                 int iters, double lambda0, double up, double down, float* params_out,
                                 double* energy_before, double* energy_after, int* accepted, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  SQR_CHECK_ARG(K >= 1 && B >= 1 && (long long)K * B <= 65535, "pts_lm_refine: K=%d x B=%d out of range [1,65535]", K,
                B);
  return lm_refine_entry("pts_lm_refine", params_in, ListSrc{points, count, B, P}, K, B, iters, lambda0, up, down,
                         params_out, energy_before, energy_after, accepted, workspace, workspace_bytes, stream);
}

// the moments' partials [B][nblk][kMomN], then the extents' [B][nblk][6], float64
static size_t starts_bytes(size_t B, size_t slots) { return B * slot_blocks(slots) * (kMomN + 6) * sizeof(double); }

extern "C" size_t sqr_lsq_starts_workspace_bytes(int B, int R) {
  if (B <= 0 || R <= 0) return 0;
  return starts_bytes((size_t)B, image_slots(R));
}

extern "C" size_t sqr_pts_starts_workspace_bytes(int B, int P) {
  if (B <= 0 || P <= 0) return 0;
  return starts_bytes((size_t)B, (size_t)P);
}

// the four launches of the starts (arguments checked by the callers)
template <class Src>
static int launch_starts(hipStream_t st, const Src& src, int B, int nsets, float e0, float depth, float* starts,
                         int* count, double* centroid, double* eigenvalues, double* frame, double* workspace) {
  const int nblk = (int)slot_blocks(src.slots());
  double* mom = workspace;
  double* ext = mom + (size_t)B * nblk * kMomN;
  hipLaunchKernelGGL((lsq_moments_kernel<256, Src>), dim3(nblk, B), dim3(256), 0, st, src, mom);
  SQR_HIP_LAUNCH_CHECK("lsq_moments_kernel");
  hipLaunchKernelGGL(lsq_frame_kernel, dim3((B + 63) / 64), dim3(64), 0, st, mom, B, nblk, count, centroid,
                     eigenvalues, frame);
  SQR_HIP_LAUNCH_CHECK("lsq_frame_kernel");
  hipLaunchKernelGGL((lsq_extents_kernel<256, Src>), dim3(nblk, B), dim3(256), 0, st, src, frame, ext);
  SQR_HIP_LAUNCH_CHECK("lsq_extents_kernel");
  hipLaunchKernelGGL(lsq_starts_kernel, dim3((3 * nsets * B + 63) / 64), dim3(64), 0, st, B, nblk, nsets, e0, depth,
                     count, frame, ext, starts);
  SQR_HIP_LAUNCH_CHECK("lsq_starts_kernel");
  return SQR_OK;
}

// nsets = 1: sqr_lsq_starts and sqr_pts_starts (depth 0), 2: sqr_lsq_starts6
template <class Src>
static int starts_entry(const char* who, const Src& src, int B, int nsets, float e0, float depth, float* starts,
                        int* count, double* centroid, double* eigenvalues, double* frame, void* workspace,
                        size_t workspace_bytes, void* stream) {
  SQR_CHECK_ARG(B >= 1 && B <= 65535, "%s: B=%d out of range [1,65535]", who, B);
  const int rc = check_source(who, src);
  if (rc != SQR_OK) return rc;
  SQR_CHECK_ARG(e0 >= 0.1f && e0 <= 1.f, "%s: e0=%g outside [0.1,1]", who, (double)e0);
  SQR_CHECK_ARG(depth >= 0.f && depth <= 8.f, "%s: depth=%g outside [0,8]", who, (double)depth);
  SQR_CHECK_ARG(starts && count && centroid && eigenvalues && frame && workspace, "%s: null pointer", who);
  const size_t need = starts_bytes((size_t)B, src.slots());
  SQR_CHECK_ARG(workspace_bytes >= need, "%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
  return launch_starts(as_stream(stream), src, B, nsets, e0, depth, starts, count, centroid, eigenvalues, frame,
                       (double*)workspace);
}

extern "C" int sqr_lsq_starts(const float* target, int B, int H, int W, int R, float e0, float* starts, int* count,
                              double* centroid, double* eigenvalues, double* frame, void* workspace,
                              size_t workspace_bytes, void* stream) {
  return starts_entry("lsq_starts", ImageSrc{target, B, H, W, R}, B, 1, e0, 0.f, starts, count, centroid, eigenvalues,
                      frame, workspace, workspace_bytes, stream);
}

extern "C" int sqr_pts_starts(const float* points, const int* count, int B, int P, float e0, float* starts,
                              int* count_out, double* centroid, double* eigenvalues, double* frame, void* workspace,
                              size_t workspace_bytes, void* stream) {
  return starts_entry("pts_starts", ListSrc{points, count, B, P}, B, 1, e0, 0.f, starts, count_out, centroid,
                      eigenvalues, frame, workspace, workspace_bytes, stream);
}

extern "C" int sqr_lsq_starts6(const float* target, int B, int H, int W, int R, float e0, float depth, float* starts,
                               int* count, double* centroid, double* eigenvalues, double* frame, void* workspace,
                               size_t workspace_bytes, void* stream) {
  return starts_entry("lsq_starts6", ImageSrc{target, B, H, W, R}, B, 2, e0, depth, starts, count, centroid,
                      eigenvalues, frame, workspace, workspace_bytes, stream);
}

extern "C" int sqr_lsq_select(int B, int K, const float* params, const double* energy, float* out_params,
                              double* out_energy, int* out_index, void* stream) {
  SQR_CHECK_ARG(B >= 1, "lsq_select: B=%d must be >= 1", B);
  SQR_CHECK_ARG(K >= 1, "lsq_select: K=%d must be >= 1", K);
  SQR_CHECK_ARG(params && energy && out_params && out_energy && out_index, "lsq_select: null pointer");
  hipLaunchKernelGGL(lsq_select_kernel, dim3((B + 63) / 64), dim3(64), 0, as_stream(stream), B, K, params, energy,
                     out_params, out_energy, out_index);
  SQR_HIP_LAUNCH_CHECK("lsq_select_kernel");
  return SQR_OK;
}

extern "C" size_t sqr_lsq_free_space_workspace_bytes(int S, int R) {
  if (S <= 0 || R <= 0) return 0;
  return (size_t)S * slot_blocks(image_slots(R)) * sizeof(double);
}

// the two launches of the free-space energy (arguments checked by the callers)
static int launch_free_space(hipStream_t st, const float* params, const float* target, int S, int B, int H, int W,
                             int R, float margin, double* energy_fs, const double* energy, double w, double* score,
                             double* partials) {
  const int nblk = (int)slot_blocks(image_slots(R));
  hipLaunchKernelGGL((free_space_kernel<256>), dim3(nblk, S), dim3(256), 0, st, params, target, B, H, W, R, margin,
                     partials);
  SQR_HIP_LAUNCH_CHECK("free_space_kernel");
  hipLaunchKernelGGL(free_space_finalize_kernel, dim3((S + 63) / 64), dim3(64), 0, st, params, partials, S, nblk,
                     energy_fs, energy, w, score);
  SQR_HIP_LAUNCH_CHECK("free_space_finalize_kernel");
  return SQR_OK;
}

extern "C" int sqr_lsq_free_space(const float* params, const float* target, int S, int B, int H, int W, int R,
                                  float margin, double* energy_fs, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  SQR_CHECK_ARG(B >= 1 && S >= B && S <= 65535 && S % B == 0,
                "lsq_free_space: S=%d must be a multiple of B=%d in [B,65535]", S, B);
  SQR_CHECK_ARG(R >= 1 && R <= 1024, "lsq_free_space: R=%d out of range [1,1024]", R);
  SQR_CHECK_ARG(H >= 1 && W >= 1, "lsq_free_space: bad target size %dx%d", H, W);
  SQR_CHECK_ARG(margin >= 0.f, "lsq_free_space: margin=%g must be >= 0", (double)margin);
  SQR_CHECK_ARG(params && target && energy_fs && workspace, "lsq_free_space: null pointer");
  const size_t need = sqr_lsq_free_space_workspace_bytes(S, R);
  SQR_CHECK_ARG(workspace_bytes >= need, "lsq_free_space: workspace %zu < %zu bytes", workspace_bytes, need);
  return launch_free_space(as_stream(stream), params, target, S, B, H, W, R, margin, energy_fs, nullptr, 0.0, nullptr,
                           (double*)workspace);
}

// -------------------------------------------------------------------------- the recovery chain
// Workspace of both recoveries, float64 first: [centroid 3][eigenvalues 3][frame 9] per image, then one region that
// the starts' partials, the batched refinement and the free-space partials (always the smallest) use in turn, then
// (sqr_lsq_recover, which does not return them) the starts [3,B,12] f32, then count [B] i32.
constexpr size_t kRecoverDoubles = 3 + 3 + 9;

static size_t recover_region_bytes(size_t K, size_t B, size_t slots) {
  const size_t a = starts_bytes(B, slots), b = lm_refine_bytes(K * B, slots);
  return a > b ? a : b;
}

static size_t recover_bytes(size_t K, size_t B, size_t slots) {
  return B * kRecoverDoubles * sizeof(double) + recover_region_bytes(K, B, slots) + B * sizeof(int);
}

extern "C" size_t sqr_lsq_recover_multi_workspace_bytes(int K, int B, int R) {
  if (K <= 0 || B <= 0 || R <= 0) return 0;
  return recover_bytes((size_t)K, (size_t)B, image_slots(R));
}

extern "C" size_t sqr_pts_recover_workspace_bytes(int K, int B, int P) {
  if (K <= 0 || B <= 0 || P <= 0) return 0;
  return recover_bytes((size_t)K, (size_t)B, (size_t)P);
}

extern "C" size_t sqr_lsq_recover_workspace_bytes(int B, int R) {
  if (B <= 0 || R <= 0) return 0;
  return sqr_lsq_recover_multi_workspace_bytes(3, B, R) + (size_t)B * 3 * 12 * sizeof(float);
}

// The scored selection's arguments and outputs (sqr_lsq_recover_multi): an image source only, a list has no rays
struct FreeSpaceSel {
  double w_fs;
  float margin;
  double *energy_fs_out, *all_fs, *all_score;
};

// The recoveries behind their own batch bounds, `who` the entry's name in the messages: the starts (nstarts = 3 or
// 6), the caller's Kx extra ones behind them, one refinement chain over all K B samples, K = nstarts + Kx, and the
// selection: scored (fs != NULL; images), on all_after + w_fs all_fs, or on all_after.  all_starts NULL: the starts
// stay in the workspace.
template <class Src>
static int recover_chain(const char* who, const FreeSpaceSel* fs, const Src& src, int B, int iters, int nstarts,
                         float e0, float depth, const float* extra, int Kx, double lambda0, double up, double down,
                         float* params_out, double* energy_out, int* index_out, float* all_starts, float* all_params,
                         double* all_before, double* all_after, int* all_accepted, void* workspace,
                         size_t workspace_bytes, void* stream) {
  const int K = nstarts + Kx;
  const size_t nb = (size_t)B, own_starts = all_starts ? 0 : (size_t)K * nb * 12 * sizeof(float);
  int rc = check_source(who, src);
  if (rc != SQR_OK) return rc;
  SQR_CHECK_ARG(iters >= 0, "%s: iters=%d must be >= 0", who, iters);
  SQR_CHECK_ARG(e0 >= 0.1f && e0 <= 1.f, "%s: e0=%g outside [0.1,1]", who, (double)e0);
  SQR_CHECK_ARG(depth >= 0.f && depth <= 8.f, "%s: depth=%g outside [0,8]", who, (double)depth);
  SQR_CHECK_ARG(lambda0 > 0.0, "%s: lambda0=%g must be > 0", who, lambda0);
  SQR_CHECK_ARG(up > 1.0, "%s: up=%g must be > 1", who, up);
  SQR_CHECK_ARG(down > 0.0 && down < 1.0, "%s: down=%g outside (0,1)", who, down);
  SQR_CHECK_ARG(!fs || (fs->w_fs >= 0.0 && fs->w_fs <= 1e300), "%s: w_fs=%g must be a finite number >= 0", who,
                fs->w_fs);
  SQR_CHECK_ARG(!fs || fs->margin >= 0.f, "%s: margin=%g must be >= 0", who, (double)fs->margin);
  SQR_CHECK_ARG(params_out && energy_out && index_out && all_params && all_before && all_after && all_accepted &&
                    workspace && (!fs || (fs->energy_fs_out && all_starts && fs->all_fs && fs->all_score)),
                "%s: null pointer", who);
  const size_t need = recover_bytes((size_t)K, nb, src.slots()) + own_starts;
  SQR_CHECK_ARG(workspace_bytes >= need, "%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
  hipStream_t st = as_stream(stream);
  double* centroid = (double*)workspace;
  double* eigenvalues = centroid + 3 * nb;
  double* frame = eigenvalues + 3 * nb;
  char* region = (char*)(frame + 9 * nb);
  char* tail = region + recover_region_bytes((size_t)K, nb, src.slots());
  if (!all_starts) all_starts = (float*)tail;
  int* count = (int*)(tail + own_starts);
  rc = launch_starts(st, src, B, nstarts / 3, e0, depth, all_starts, count, centroid, eigenvalues, frame,
                     (double*)region);
  if (rc != SQR_OK) return rc;
  if (Kx > 0) {
    const long long n = (long long)Kx * B * 12;
    hipLaunchKernelGGL(lsq_copy_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, extra, n,
                       all_starts + 12 * nb * nstarts);
    SQR_HIP_LAUNCH_CHECK("lsq_copy_kernel");
  }
  rc = lm_refine_chain(all_starts, src, K * B, iters, lambda0, up, down, all_params, all_before, all_after,
                       all_accepted, region, stream);
  if (rc != SQR_OK) return rc;
  if constexpr (std::is_same<Src, ImageSrc>::value) {
    if (fs) {
      rc = launch_free_space(st, all_params, src.target, K * B, B, src.H, src.W, src.R, fs->margin, fs->all_fs,
                             all_after, fs->w_fs, fs->all_score, (double*)region);
      if (rc != SQR_OK) return rc;
      // the winning score goes to energy_out first; the gather puts the winner's point energy there
      rc = sqr_lsq_select(B, K, all_params, fs->all_score, params_out, energy_out, index_out, stream);
      if (rc != SQR_OK) return rc;
      hipLaunchKernelGGL(lsq_gather_kernel, dim3((B + 63) / 64), dim3(64), 0, st, B, index_out, all_after, fs->all_fs,
                         energy_out, fs->energy_fs_out);
      SQR_HIP_LAUNCH_CHECK("lsq_gather_kernel");
      return SQR_OK;
    }
  }
  return sqr_lsq_select(B, K, all_params, all_after, params_out, energy_out, index_out, stream);
}

extern "C" int sqr_lsq_recover(const float* target, int B, int H, int W, int R, int iters, float e0, double lambda0,
                               double up, double down, float* params_out, double* energy_out, int* index_out,
                               float* all_params, double* all_before, double* all_after, int* all_accepted,
                               void* workspace, size_t workspace_bytes, void* stream) {
  // 3 B samples in one chain: gridDim.y of its launches
  SQR_CHECK_ARG(B >= 1 && 3LL * B <= 65535, "lsq_recover: K=3 x B=%d out of range [1,65535]", B);
  return recover_chain("lsq_recover", nullptr, ImageSrc{target, B, H, W, R}, B, iters, 3, e0, 0.f, nullptr, 0, lambda0,
                       up, down, params_out, energy_out, index_out, nullptr, all_params, all_before, all_after,
                       all_accepted, workspace, workspace_bytes, stream);
}

extern "C" int sqr_pts_recover(const float* points, const int* count, int B, int P, int iters, float e0,
                               const float* extra, int Kx, double lambda0, double up, double down, float* params_out,
                               double* energy_out, int* index_out, float* all_starts, float* all_params,
                               double* all_before, double* all_after, int* all_accepted, void* workspace,
                               size_t workspace_bytes, void* stream) {
  SQR_CHECK_ARG(Kx >= 0 && (Kx == 0 || extra), "pts_recover: Kx=%d extra starts without a pointer", Kx);
  const long long K = 3LL + Kx;
  SQR_CHECK_ARG(B >= 1 && K * B <= 65535, "pts_recover: K=%lld x B=%d out of range [1,65535]", K, B);
  SQR_CHECK_ARG(all_starts, "pts_recover: null pointer");
  return recover_chain("pts_recover", nullptr, ListSrc{points, count, B, P}, B, iters, 3, e0, 0.f, extra, Kx, lambda0,
                       up, down, params_out, energy_out, index_out, all_starts, all_params, all_before, all_after,
                       all_accepted, workspace, workspace_bytes, stream);
}

extern "C" int sqr_lsq_recover_multi(const float* target, int B, int H, int W, int R, int iters, int nstarts, float e0,
                                     float depth, const float* extra, int Kx, double lambda0, double up, double down,
                                     double w_fs, float margin, float* params_out, double* energy_out,
                                     double* energy_fs_out, int* index_out, float* all_starts, float* all_params,
                                     double* all_before, double* all_after, double* all_fs, double* all_score,
                                     int* all_accepted, void* workspace, size_t workspace_bytes, void* stream) {
  SQR_CHECK_ARG(nstarts == 3 || nstarts == 6, "lsq_recover_multi: nstarts=%d must be 3 or 6", nstarts);
  SQR_CHECK_ARG(Kx >= 0 && (Kx == 0 || extra), "lsq_recover_multi: Kx=%d extra starts without a pointer", Kx);
  const long long K = (long long)nstarts + Kx;
  SQR_CHECK_ARG(B >= 1 && K * B <= 65535, "lsq_recover_multi: K=%lld x B=%d out of range [1,65535]", K, B);
  const FreeSpaceSel fs{w_fs, margin, energy_fs_out, all_fs, all_score};
  return recover_chain("lsq_recover_multi", &fs, ImageSrc{target, B, H, W, R}, B, iters, nstarts, e0, depth, extra, Kx,
                       lambda0, up, down, params_out, energy_out, index_out, all_starts, all_params, all_before,
                       all_after, all_accepted, workspace, workspace_bytes, stream);
}


// -------------------------------------------------------------------------- several parts per cloud (C ABI)
// B clouds of M parts: 3 B M samples are one recovery chain's gridDim.y
static int check_parts(const char* who, int B, int P, int M) {
  SQR_CHECK_ARG(M >= 1 && M <= kMaxParts, "%s: M=%d out of range [1,%d]", who, M, kMaxParts);
  SQR_CHECK_ARG(B >= 1 && 3LL * B * M <= 65535, "%s: 3 x B=%d x M=%d out of range [1,65535]", who, B, M);
  SQR_CHECK_ARG(P >= 1 && P <= kMaxListSlots, "%s: P=%d out of range [1,%d]", who, P, kMaxListSlots);
  return SQR_OK;
}

// the assignment's per-block partials: pdist [B][nblk][M] f64, pcount [B][nblk][M] i32, pchanged [B][nblk] i32
static size_t assign_bytes(size_t B, size_t P, size_t M) {
  const size_t n = B * slot_blocks(P);
  return (n * M * (sizeof(double) + sizeof(int)) + n * sizeof(int) + 7) / 8 * 8;
}

extern "C" size_t sqr_pts_assign_workspace_bytes(int B, int P, int M) {
  if (B <= 0 || P <= 0 || M <= 0) return 0;
  return assign_bytes((size_t)B, (size_t)P, (size_t)M);
}

// the assignment's launches (arguments checked by the callers); part_count NULL: no finalize (the Lloyd iterations)
template <bool kCentre>
static int launch_assign(hipStream_t st, const float* points, const int* count, int B, int P, int M,
                         const float* rows, const int* prev, int* label, float* dist, int* part_count,
                         double* part_dist, int* changed, void* workspace) {
  const int nblk = (int)slot_blocks((size_t)P);
  double* pdist = (double*)workspace;
  int* pcount = (int*)(pdist + (size_t)B * nblk * M);
  int* pchanged = pcount + (size_t)B * nblk * M;
  hipLaunchKernelGGL((pts_assign_kernel<256, kCentre>), dim3(nblk, B), dim3(256), 0, st, points, count, B, P, M, rows,
                     prev, label, dist, pdist, pcount, pchanged);
  SQR_HIP_LAUNCH_CHECK("pts_assign_kernel");
  if (!part_count) return SQR_OK;
  hipLaunchKernelGGL(pts_assign_finalize_kernel, dim3((B * M + 63) / 64), dim3(64), 0, st, B, M, nblk, pdist, pcount,
                     pchanged, part_count, part_dist, prev ? changed : nullptr);
  SQR_HIP_LAUNCH_CHECK("pts_assign_finalize_kernel");
  return SQR_OK;
}

extern "C" int sqr_pts_assign(const float* points, const int* count, const float* params, const int* label_prev,
                              int B, int P, int M, int* label, float* dist, int* part_count, double* part_dist,
                              int* changed, void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = check_parts("pts_assign", B, P, M);
  if (rc != SQR_OK) return rc;
  SQR_CHECK_ARG(points && params && label && dist && part_count && part_dist && workspace && (!label_prev || changed),
                "pts_assign: null pointer");
  SQR_CHECK_ARG(label_prev != label, "pts_assign: label and label_prev are the same buffer");
  const size_t need = assign_bytes((size_t)B, (size_t)P, (size_t)M);
  SQR_CHECK_ARG(workspace_bytes >= need, "pts_assign: workspace %zu < %zu bytes", workspace_bytes, need);
  return launch_assign<false>(as_stream(stream), points, count, B, P, M, params, label_prev, label, dist, part_count,
                              part_dist, changed, workspace);
}

// The seeding's workspace: mind [B,P] f32 (the Lloyd assignments' dist afterwards), the assignment's partials, the
// moments' partials [B M][nblk][kMomN] f64
static size_t seed_bytes(size_t B, size_t P, size_t M) {
  return (B * P * sizeof(float) + 7) / 8 * 8 + assign_bytes(B, P, M) + B * M * slot_blocks(P) * kMomN * sizeof(double);
}

extern "C" size_t sqr_pts_seed_workspace_bytes(int B, int P, int M) {
  if (B <= 0 || P <= 0 || M <= 0) return 0;
  return seed_bytes((size_t)B, (size_t)P, (size_t)M);
}

// the seeding's launches (arguments checked by the callers): 2 + 3 lloyd
static int launch_seed(hipStream_t st, const float* points, const int* count, int B, int P, int M, int lloyd,
                       int* label, float* centres, int* seeds, void* workspace) {
  const int nblk = (int)slot_blocks((size_t)P);
  float* mind = (float*)workspace;
  char* asg = (char*)workspace + ((size_t)B * P * sizeof(float) + 7) / 8 * 8;
  double* mom = (double*)(asg + assign_bytes((size_t)B, (size_t)P, (size_t)M));
  hipLaunchKernelGGL((pts_fps_kernel<256>), dim3(B), dim3(256), 0, st, points, count, B, P, M, mind, seeds, centres);
  SQR_HIP_LAUNCH_CHECK("pts_fps_kernel");
  int rc = launch_assign<true>(st, points, count, B, P, M, centres, nullptr, label, mind, nullptr, nullptr, nullptr,
                               asg);
  if (rc != SQR_OK) return rc;
  const PartSrc src{points, count, label, B, P, M};
  for (int it = 0; it < lloyd; ++it) {
    hipLaunchKernelGGL((lsq_moments_kernel<256, PartSrc>), dim3(nblk, B * M), dim3(256), 0, st, src, mom);
    SQR_HIP_LAUNCH_CHECK("lsq_moments_kernel");
    hipLaunchKernelGGL(pts_centre_kernel, dim3((B * M + 63) / 64), dim3(64), 0, st, B * M, nblk, mom, centres);
    SQR_HIP_LAUNCH_CHECK("pts_centre_kernel");
    rc = launch_assign<true>(st, points, count, B, P, M, centres, nullptr, label, mind, nullptr, nullptr, nullptr, asg);
    if (rc != SQR_OK) return rc;
  }
  return SQR_OK;
}

extern "C" int sqr_pts_seed(const float* points, const int* count, int B, int P, int M, int lloyd, int* label,
                            float* centres, int* seeds, void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = check_parts("pts_seed", B, P, M);
  if (rc != SQR_OK) return rc;
  SQR_CHECK_ARG(lloyd >= 0, "pts_seed: lloyd=%d must be >= 0", lloyd);
  SQR_CHECK_ARG(points && label && centres && seeds && workspace, "pts_seed: null pointer");
  const size_t need = seed_bytes((size_t)B, (size_t)P, (size_t)M);
  SQR_CHECK_ARG(workspace_bytes >= need, "pts_seed: workspace %zu < %zu bytes", workspace_bytes, need);
  return launch_seed(as_stream(stream), points, count, B, P, M, lloyd, label, centres, seeds, workspace);
}

extern "C" size_t sqr_pts_labeled_lm_refine_workspace_bytes(int S, int P) { return sqr_pts_lm_refine_workspace_bytes(S, P); }

extern "C" int sqr_pts_labeled_lm_refine(const float* params_in, const float* points, const int* count,
                                         const int* label, int K, int B, int P, int M, int iters, double lambda0,
                                         double up, double down, float* params_out, double* energy_before,
                                         double* energy_after, int* accepted, void* workspace, size_t workspace_bytes,
                                         void* stream) {
  SQR_CHECK_ARG(K >= 1 && B >= 1 && M >= 1 && (long long)K * B * M <= 65535,
                "pts_labeled_lm_refine: K=%d x B=%d x M=%d out of range [1,65535]", K, B, M);
  return lm_refine_entry("pts_labeled_lm_refine", params_in, PartSrc{points, count, label, B, P, M}, K, B * M, iters,
                         lambda0, up, down, params_out, energy_before, energy_after, accepted, workspace,
                         workspace_bytes, stream);
}

extern "C" size_t sqr_pts_labeled_recover_workspace_bytes(int K, int S, int P) {
  return sqr_pts_recover_workspace_bytes(K, S, P);
}

extern "C" int sqr_pts_labeled_recover(const float* points, const int* count, const int* label, int B, int P, int M,
                                       int iters, float e0, const float* extra, int Kx, double lambda0, double up,
                                       double down, float* params_out, double* energy_out, int* index_out,
                                       float* all_starts, float* all_params, double* all_before, double* all_after,
                                       int* all_accepted, void* workspace, size_t workspace_bytes, void* stream) {
  SQR_CHECK_ARG(Kx >= 0 && (Kx == 0 || extra), "pts_labeled_recover: Kx=%d extra starts without a pointer", Kx);
  const long long K = 3LL + Kx;
  SQR_CHECK_ARG(B >= 1 && M >= 1 && K * B * M <= 65535, "pts_labeled_recover: K=%lld x B=%d x M=%d out of range [1,65535]",
                K, B, M);
  SQR_CHECK_ARG(all_starts, "pts_labeled_recover: null pointer");
  return recover_chain("pts_labeled_recover", nullptr, PartSrc{points, count, label, B, P, M}, B * M, iters, 3, e0, 0.f,
                       extra, Kx, lambda0, up, down, params_out, energy_out, index_out, all_starts, all_params,
                       all_before, all_after, all_accepted, workspace, workspace_bytes, stream);
}

// sqr_pts_recover_parts' workspace over S = B M parts: the second label and parameter buffers (the rounds alternate
// between them and the outputs), round 0's per-start outputs (all_params [3,S,12] f32, all_before / all_after [3,S]
// f64, all_accepted [3,S] i32, index [S] i32; the later rounds' energy_before and accepted lie in them), the
// assignment's partials, and one region that the seeding and the recovery chain (its starts inside) use in turn
struct PartsLayout {
  size_t label2, params2, all_before, all_after, all_params, all_accepted, index, assign, region, region_bytes, total;
};

static PartsLayout parts_layout(size_t B, size_t P, size_t M) {
  const size_t S = B * M;
  auto up8 = [](size_t n) { return (n + 7) / 8 * 8; };
  PartsLayout l;
  size_t at = 0;
  l.all_before = at; at += 3 * S * sizeof(double);
  l.all_after = at;  at += 3 * S * sizeof(double);
  l.assign = at;     at += assign_bytes(B, P, M);
  l.region = at;
  const size_t rec = recover_bytes(3, S, P) + 3 * S * 12 * sizeof(float), sd = seed_bytes(B, P, M);
  l.region_bytes = up8(rec > sd ? rec : sd);
  at += l.region_bytes;
  l.label2 = at;       at += up8(B * P * sizeof(int));
  l.params2 = at;      at += up8(S * 12 * sizeof(float));
  l.all_params = at;   at += up8(3 * S * 12 * sizeof(float));
  l.all_accepted = at; at += up8(3 * S * sizeof(int));
  l.index = at;        at += up8(S * sizeof(int));
  l.total = at;
  return l;
}

extern "C" size_t sqr_pts_recover_parts_workspace_bytes(int B, int P, int M) {
  if (B <= 0 || P <= 0 || M <= 0) return 0;
  return parts_layout((size_t)B, (size_t)P, (size_t)M).total;
}

extern "C" int sqr_pts_recover_parts(const float* points, const int* count, const int* label_in, int B, int P, int M,
                                     int rounds, int iters0, int iters, int lloyd, float e0, double lambda0, double up,
                                     double down, float* params_out, int* label_out, double* energy_out,
                                     float* dist, int* part_count, double* part_dist, int* changed, int* seeds,
                                     float* centres, void* workspace, size_t workspace_bytes, void* stream) {
  int rc = check_parts("pts_recover_parts", B, P, M);
  if (rc != SQR_OK) return rc;
  SQR_CHECK_ARG(rounds >= 1 && rounds <= 1024, "pts_recover_parts: rounds=%d out of range [1,1024]", rounds);
  SQR_CHECK_ARG(iters0 >= 0 && iters >= 0, "pts_recover_parts: iters0=%d, iters=%d must be >= 0", iters0, iters);
  SQR_CHECK_ARG(lloyd >= 0, "pts_recover_parts: lloyd=%d must be >= 0", lloyd);
  SQR_CHECK_ARG(e0 >= 0.1f && e0 <= 1.f, "pts_recover_parts: e0=%g outside [0.1,1]", (double)e0);
  SQR_CHECK_ARG(lambda0 > 0.0, "pts_recover_parts: lambda0=%g must be > 0", lambda0);
  SQR_CHECK_ARG(up > 1.0, "pts_recover_parts: up=%g must be > 1", up);
  SQR_CHECK_ARG(down > 0.0 && down < 1.0, "pts_recover_parts: down=%g outside (0,1)", down);
  SQR_CHECK_ARG(points && params_out && label_out && energy_out && dist && part_count && part_dist && changed &&
                    workspace && (label_in || (seeds && centres)),
                "pts_recover_parts: null pointer");
  SQR_CHECK_ARG(label_in != label_out, "pts_recover_parts: label_in and label_out are the same buffer");
  const PartsLayout l = parts_layout((size_t)B, (size_t)P, (size_t)M);
  SQR_CHECK_ARG(workspace_bytes >= l.total, "pts_recover_parts: workspace %zu < %zu bytes", workspace_bytes, l.total);
  hipStream_t st = as_stream(stream);
  char* ws = (char*)workspace;
  const int S = B * M;
  double* all_before = (double*)(ws + l.all_before);
  double* all_after = (double*)(ws + l.all_after);
  float* all_params = (float*)(ws + l.all_params);
  int* all_accepted = (int*)(ws + l.all_accepted);
  int* index = (int*)(ws + l.index);
  // round t writes labels and parameters into buffer (rounds - 1 - t) & 1: 0 the outputs, 1 the workspace's, so
  // that the last round ends in the outputs and no round reads what it writes
  int* lbuf[2] = {label_out, (int*)(ws + l.label2)};
  float* pbuf[2] = {params_out, (float*)(ws + l.params2)};
  const int* cur = label_in;
  if (!cur) {
    int* first = lbuf[rounds & 1];
    rc = launch_seed(st, points, count, B, P, M, lloyd, first, centres, seeds, ws + l.region);
    if (rc != SQR_OK) return rc;
    cur = first;
  }
  for (int t = 0; t < rounds; ++t) {
    const int w = (rounds - 1 - t) & 1;
    const PartSrc src{points, count, cur, B, P, M};
    if (t == 0) {
      rc = recover_chain("pts_recover_parts", nullptr, src, S, iters0, 3, e0, 0.f, nullptr, 0, lambda0, up, down,
                         pbuf[w], energy_out, index, nullptr, all_params, all_before, all_after, all_accepted,
                         ws + l.region, l.region_bytes, stream);
    } else {
      rc = lm_refine_chain(pbuf[w ^ 1], src, S, iters, lambda0, up, down, pbuf[w], all_before, energy_out,
                           all_accepted, ws + l.region, stream);
    }
    if (rc != SQR_OK) return rc;
    rc = launch_assign<false>(st, points, count, B, P, M, pbuf[w], cur, lbuf[w], dist, part_count, part_dist,
                              changed + (size_t)t * B, ws + l.assign);
    if (rc != SQR_OK) return rc;
    cur = lbuf[w];
  }
  return SQR_OK;
}
