// kfn_pnp.hip -- camera poses from the scene-coordinate records: batched RANSAC-PnP on the device.
//
// The reference stops at coord_<i>.npy and points to an external PnP program (README.md:132-138) that it ships only as a
// git-lfs pointer.  Here the whole estimate stays on the device; DESIGN.md "Camera poses" fixes every step so that the
// numpy restatement in tests/pnp_ref.py draws the same samples and solves the same P3P:
//   1. pnp_hyp_kernel     one workgroup per (frame, 256 hypotheses): the frame's candidate list (raster order) is built in
//                         LDS, then one lane per hypothesis draws its 4 indices from a counter-based hash and solves P3P
//                         in fp64 (Grunert's quartic, Ferrari's roots); R|t goes out in fp32, the count is set to 0 (valid)
//                         or -1 (invalid).
//   2. pnp_score_kernel   the hot path: a grid of (cell tile, hypothesis block, frame).  A tile's candidates are compacted
//                         into LDS (X, Y, Z, pixel - principal point); every lane holds one hypothesis in registers and
//                         reads the points as broadcasts; the tile's integer inlier count is added to the hypothesis'
//                         count with an atomic (integer addition: the order does not matter).
//   3. pnp_refine_kernel  one workgroup per frame: the best hypothesis (ties to the lowest index), then Gauss-Newton on the
//                         pixel error over the inliers of the current pose, normal equations in fp64 reduced in a fixed
//                         order (per-lane strided sums, a butterfly per wave, the four waves in order).
//      pnp_refine_unc_kernel   its sibling behind kfn_pnp_ransac_unc: optionally weighted by the records' sigma propagated
//                         to the image plane; also writes the pose's 6x6 covariance and (cost, degrees of freedom).
//   kfn_pnp_ransac_guided runs pnp_cdf_kernel (per frame: integer weights from the confidence, their cumulative sums in
//                         uint64) and pnp_hyp_guided_kernel (stage 1 with every draw taken from those sums) in front of
//                         stages 2 and 3: DESIGN.md 5c "Guided sampling".
// No host round trip between the stages, no device RNG state, no float atomics: the result is the same bits on every launch.
#include <cmath>

#include "kfn_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int NT = 256;          // threads of every workgroup here; the hypothesis block of one lane per hypothesis
constexpr int TILE = 128;        // grid cells per scoring workgroup
constexpr int MAX_DRAWS = 16;
constexpr int MAX_CELLS = 32768; // the candidate list is uint16 cell indices in LDS: 64 KiB

struct PnPArgs {
  const float* rec;
  int B, h, w, ld, t0;
  uint32_t seed;
  int H, iters, min_points;
  float fx, fy, u, v;
  int cs;
  float minc, thr;
};

__device__ __forceinline__ uint32_t lowbias32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

__device__ __forceinline__ bool is_candidate(const float* p, float minc) {
  return p[3] > minc && isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
}

// The frame's candidates as cell indices in raster order (order-preserving: ballot prefix within a wave, wave totals in
// order).  Every thread of the 256-thread block takes part; returns n in every thread.
__device__ int build_candidates(const PnPArgs& a, const float* r, unsigned short* list, int* wave_tot) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int hw = a.h * a.w;
  int base = 0;
  for (int c0 = 0; c0 < hw; c0 += NT) {
    const int c = c0 + tid;
    const bool keep = c < hw && is_candidate(r + (size_t)c * a.ld, a.minc);
    const unsigned long long m = __ballot(keep);
    const int pre = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_tot[wv] = __popcll(m);
    __syncthreads();
    int off = base;
    for (int k = 0; k < wv; ++k) off += wave_tot[k];
    if (keep) list[off + pre] = (unsigned short)c;
    base += (wave_tot[0] + wave_tot[1]) + (wave_tot[2] + wave_tot[3]);
    __syncthreads();
  }
  return base;
}

// ---- P3P: Grunert's quartic (Haralick et al., IJCV 1994) with Ferrari's roots, fp64 -----------------------------------

__device__ double cubic_largest_root(double a, double b, double c) {
  const double P = b - a * a / 3.0;
  const double Q = 2.0 * a * a * a / 27.0 - a * b / 3.0 + c;
  const double D = Q * Q / 4.0 + P * P * P / 27.0;
  double z;
  if (D >= 0.0) {
    const double sd = sqrt(D);
    z = cbrt(-Q / 2.0 + sd) + cbrt(-Q / 2.0 - sd);
  } else {
    double k = 3.0 * Q / (2.0 * P) * sqrt(-3.0 / P);
    k = fmin(1.0, fmax(-1.0, k));
    z = 2.0 * sqrt(-P / 3.0) * cos(acos(k) / 3.0);
  }
  double m = z - a / 3.0;
  for (int i = 0; i < 2; ++i) {
    const double f = ((m + a) * m + b) * m + c;
    const double df = (3.0 * m + 2.0 * a) * m + b;
    if (df != 0.0) m -= f / df;
  }
  return m;
}

__device__ __forceinline__ void quadratic(double B, double C, double* out, int& n) {
  double d = B * B - 4.0 * C;
  if (d < 0.0) {
    if (d < -1e-10 * fmax(1.0, B * B)) return;
    d = 0.0;
  }
  const double s = sqrt(d);
  out[n++] = (-B + s) / 2.0;
  out[n++] = (-B - s) / 2.0;
}

__device__ int solve_quartic(double A4, double A3, double A2, double A1, double A0, double* x) {
  if (fabs(A4) < 1e-14 * fmax(fmax(fmax(fabs(A3), fabs(A2)), fmax(fabs(A1), fabs(A0))), 1e-300)) return 0;
  const double b = A3 / A4, c = A2 / A4, d = A1 / A4, e = A0 / A4;
  const double p = c - 3.0 * b * b / 8.0;
  const double q = d - b * c / 2.0 + b * b * b / 8.0;
  const double r = e - b * d / 4.0 + b * b * c / 16.0 - 3.0 * b * b * b * b / 256.0;
  const double m = cubic_largest_root(p, p * p / 4.0 - r, -q * q / 8.0);
  double y[4];
  int n = 0;
  if (m > 1e-12) {
    const double s = sqrt(2.0 * m);
    quadratic(-s, p / 2.0 + m + q / (2.0 * s), y, n);
    quadratic(s, p / 2.0 + m - q / (2.0 * s), y, n);
  } else {   // q ~ 0: biquadratic y^4 + p y^2 + r
    double zz[2];
    int nz = 0;
    quadratic(p, r, zz, nz);
    for (int i = 0; i < nz; ++i)
      if (zz[i] >= 0.0) {
        y[n++] = sqrt(zz[i]);
        y[n++] = -sqrt(zz[i]);
      }
  }
  for (int i = 0; i < n; ++i) {
    double xi = y[i] - b / 4.0;
    for (int k = 0; k < 2; ++k) {
      const double f = (((xi + b) * xi + c) * xi + d) * xi + e;
      const double df = ((4.0 * xi + 3.0 * b) * xi + 2.0 * c) * xi + d;
      if (df != 0.0) xi -= f / df;
    }
    x[i] = xi;
  }
  return n;
}

__device__ __forceinline__ double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

__device__ __forceinline__ void cross3(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// orthonormal frame of a triangle, as columns F[row*3 + col]: e1 along p2-p1, e3 its normal, e2 = e3 x e1
__device__ void tri_frame(const double* p1, const double* p2, const double* p3, double* F) {
  double e1[3], d3[3], e3[3], e2[3];
  for (int i = 0; i < 3; ++i) { e1[i] = p2[i] - p1[i]; d3[i] = p3[i] - p1[i]; }
  cross3(e1, d3, e3);
  const double n1 = sqrt(dot3(e1, e1)), n3 = sqrt(dot3(e3, e3));
  for (int i = 0; i < 3; ++i) { e1[i] /= n1; e3[i] /= n3; }
  cross3(e3, e1, e2);
  for (int i = 0; i < 3; ++i) { F[i * 3 + 0] = e1[i]; F[i * 3 + 1] = e2[i]; F[i * 3 + 2] = e3[i]; }
}

__device__ __forceinline__ void load_point(const PnPArgs& a, const float* r, int cell, double* X, double* px) {
  const float* p = r + (size_t)cell * a.ld;
  X[0] = p[0]; X[1] = p[1]; X[2] = p[2];
  const int row = cell / a.w, col = cell - row * a.w;
  px[0] = (double)(a.cs * col);
  px[1] = (double)(a.cs * row);
}

// P3P on points 0..2, the solution that puts point 3 in front of the camera with the smallest pixel error (first on ties).
// Returns false if there is none.  Pose: Xc = R X + t, R row-major.
__device__ bool p3p_hypothesis(const PnPArgs& a, const double (*X)[3], const double (*px)[2], double* R, double* t) {
  const double fx = a.fx, fy = a.fy, u0 = a.u, v0 = a.v;
  double F[3][3];
  for (int i = 0; i < 3; ++i) {
    F[i][0] = (px[i][0] - u0) / fx;
    F[i][1] = (px[i][1] - v0) / fy;
    F[i][2] = 1.0;
    const double nn = sqrt(dot3(F[i], F[i]));
    for (int k = 0; k < 3; ++k) F[i][k] /= nn;
  }
  double d12[3], d02[3], d01[3];
  for (int k = 0; k < 3; ++k) { d12[k] = X[1][k] - X[2][k]; d02[k] = X[0][k] - X[2][k]; d01[k] = X[0][k] - X[1][k]; }
  const double a2 = dot3(d12, d12), b2 = dot3(d02, d02), c2 = dot3(d01, d01);
  if (b2 <= 0.0) return false;
  const double ca = dot3(F[1], F[2]), cb = dot3(F[0], F[2]), cg = dot3(F[0], F[1]);
  const double K1 = (a2 - c2) / b2, K2 = (a2 + c2) / b2;
  const double A4 = (K1 - 1.0) * (K1 - 1.0) - 4.0 * c2 / b2 * ca * ca;
  const double A3 = 4.0 * (K1 * (1.0 - K1) * cb - (1.0 - K2) * ca * cg + 2.0 * c2 / b2 * ca * ca * cb);
  const double A2 = 2.0 * (K1 * K1 - 1.0 + 2.0 * K1 * K1 * cb * cb + 2.0 * (b2 - c2) / b2 * ca * ca -
                           4.0 * K2 * ca * cb * cg + 2.0 * (b2 - a2) / b2 * cg * cg);
  const double A1 = 4.0 * (-K1 * (1.0 + K1) * cb + 2.0 * a2 / b2 * cg * cg * cb - (1.0 - K2) * ca * cg);
  const double A0 = (1.0 + K1) * (1.0 + K1) - 4.0 * a2 / b2 * cg * cg;
  double roots[4];
  const int nr = solve_quartic(A4, A3, A2, A1, A0, roots);
  double Fp[9];
  tri_frame(X[0], X[1], X[2], Fp);
  bool found = false;
  double best_e = INFINITY;
  for (int i = 0; i < nr; ++i) {
    const double v = roots[i];
    const double den = 2.0 * (cg - v * ca);
    if (v <= 0.0 || fabs(den) < 1e-12) continue;
    const double uu = ((K1 - 1.0) * v * v - 2.0 * K1 * cb * v + 1.0 + K1) / den;
    const double q = 1.0 + v * v - 2.0 * v * cb;
    if (uu <= 0.0 || q <= 0.0) continue;
    const double s1 = sqrt(b2 / q);
    double C[3][3];
    for (int k = 0; k < 3; ++k) { C[0][k] = s1 * F[0][k]; C[1][k] = uu * s1 * F[1][k]; C[2][k] = v * s1 * F[2][k]; }
    double Fc[9], Rs[9], ts[3];
    tri_frame(C[0], C[1], C[2], Fc);
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c)
        Rs[r * 3 + c] = Fc[r * 3 + 0] * Fp[c * 3 + 0] + Fc[r * 3 + 1] * Fp[c * 3 + 1] + Fc[r * 3 + 2] * Fp[c * 3 + 2];
    for (int r = 0; r < 3; ++r) ts[r] = C[0][r] - (Rs[r * 3 + 0] * X[0][0] + Rs[r * 3 + 1] * X[0][1] + Rs[r * 3 + 2] * X[0][2]);
    double xc[3];
    for (int r = 0; r < 3; ++r) xc[r] = (Rs[r * 3 + 0] * X[3][0] + Rs[r * 3 + 1] * X[3][1] + Rs[r * 3 + 2] * X[3][2]) + ts[r];
    if (!(xc[2] > 0.0)) continue;
    const double ex = fx * xc[0] / xc[2] - (px[3][0] - u0), ey = fy * xc[1] / xc[2] - (px[3][1] - v0);
    const double e2 = ex * ex + ey * ey;
    if (e2 < best_e) {
      best_e = e2;
      found = true;
      for (int k = 0; k < 9; ++k) R[k] = Rs[k];
      for (int k = 0; k < 3; ++k) t[k] = ts[k];
    }
  }
  return found;
}

// grid (ceil(H / 256), B); dynamic LDS: the uint16 candidate list
__global__ __launch_bounds__(NT) void pnp_hyp_kernel(PnPArgs a, int* __restrict__ samples, float* __restrict__ hp,
                                                     int* __restrict__ counts) {
  extern __shared__ unsigned short list[];
  __shared__ int wave_tot[NT / 64];
  const int b = blockIdx.y;
  const int k = blockIdx.x * NT + threadIdx.x;
  const float* r = a.rec + (size_t)b * a.h * a.w * a.ld;
  const int n = build_candidates(a, r, list, wave_tot);
  if (k >= a.H) return;
  int s[4] = {-1, -1, -1, -1};
  int got = 0;
  if (n >= a.min_points) {
    const uint32_t frame = (uint32_t)(a.t0 + b);
    const uint32_t key = a.seed ^ (frame * 0x9E3779B1u) ^ ((uint32_t)k * 0x85EBCA77u);
    for (int draw = 0; draw < MAX_DRAWS && got < 4; ++draw) {
      const uint32_t hsh = lowbias32(key ^ ((uint32_t)draw * 0xC2B2AE3Du));
      const int idx = (int)(((uint64_t)hsh * (uint64_t)n) >> 32);
      bool dup = false;
      for (int i = 0; i < got; ++i) dup |= s[i] == idx;
      if (!dup) s[got++] = idx;
    }
  }
  const bool sampled = got == 4;
  const size_t hk = (size_t)b * a.H + k;
  if (samples)
    for (int i = 0; i < 4; ++i) samples[hk * 4 + i] = sampled ? s[i] : -1;
  double R[9], t[3];
  bool ok = false;
  if (sampled) {
    double X[4][3], px[4][2];
    for (int i = 0; i < 4; ++i) load_point(a, r, list[s[i]], X[i], px[i]);
    ok = p3p_hypothesis(a, X, px, R, t);
  }
  float* o = hp + hk * 12;
  for (int rr = 0; rr < 3; ++rr) {
    for (int c = 0; c < 3; ++c) o[rr * 4 + c] = ok ? (float)R[rr * 3 + c] : __builtin_nanf("");
    o[rr * 4 + 3] = ok ? (float)t[rr] : __builtin_nanf("");
  }
  counts[hk] = ok ? 0 : -1;
}

// grid (ceil(h*w / TILE), ceil(H / 256), B).  Inlier test in fp32 without a division:
// ex = fx Xc - (x - u) Zc, ey = fy Yc - (y - v) Zc; inlier iff Zc > 0 and ex^2 + ey^2 < thr^2 Zc^2.
__global__ __launch_bounds__(NT) void pnp_score_kernel(PnPArgs a, const float* __restrict__ hp, int* __restrict__ counts) {
  __shared__ f32x4 sp[TILE];      // X, Y, Z, x - u
  __shared__ float sq[TILE];      // y - v
  __shared__ int wave_tot[NT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int b = blockIdx.z;
  const int hw = a.h * a.w;
  const float* r = a.rec + (size_t)b * hw * a.ld;
  const int c = blockIdx.x * TILE + tid;
  f32x4 P = {0.f, 0.f, 0.f, 0.f};
  float qy = 0.f;
  bool keep = false;
  if (tid < TILE && c < hw) {
    const float* p = r + (size_t)c * a.ld;
    keep = is_candidate(p, a.minc);
    const int row = c / a.w, col = c - row * a.w;
    P = f32x4{p[0], p[1], p[2], (float)(a.cs * col) - a.u};
    qy = (float)(a.cs * row) - a.v;
  }
  const unsigned long long m = __ballot(keep);
  if (lane == 0) wave_tot[wv] = __popcll(m);
  __syncthreads();
  int off = 0;
  for (int k = 0; k < wv; ++k) off += wave_tot[k];
  if (keep) {
    const int j = off + __popcll(m & ((1ull << lane) - 1ull));
    sp[j] = P;
    sq[j] = qy;
  }
  const int nt = (wave_tot[0] + wave_tot[1]) + (wave_tot[2] + wave_tot[3]);
  __syncthreads();
  const int k = blockIdx.y * NT + tid;
  if (nt == 0 || k >= a.H) return;
  const size_t hk = (size_t)b * a.H + k;
  if (counts[hk] < 0) return;
  const float* o = hp + hk * 12;
  const float r00 = o[0], r01 = o[1], r02 = o[2], tx = o[3];
  const float r10 = o[4], r11 = o[5], r12 = o[6], ty = o[7];
  const float r20 = o[8], r21 = o[9], r22 = o[10], tz = o[11];
  const float fx = a.fx, fy = a.fy, thr2 = a.thr * a.thr;
  int cnt = 0;
  for (int j = 0; j < nt; ++j) {
    const f32x4 q = sp[j];
    const float dy = sq[j];
    const float xc = fmaf(r00, q.x, fmaf(r01, q.y, fmaf(r02, q.z, tx)));
    const float yc = fmaf(r10, q.x, fmaf(r11, q.y, fmaf(r12, q.z, ty)));
    const float zc = fmaf(r20, q.x, fmaf(r21, q.y, fmaf(r22, q.z, tz)));
    const float ex = fmaf(fx, xc, -q.w * zc);
    const float ey = fmaf(fy, yc, -dy * zc);
    cnt += (zc > 0.f && fmaf(ex, ex, ey * ey) < thr2 * (zc * zc)) ? 1 : 0;
  }
  if (cnt) atomicAdd(&counts[hk], cnt);
}

// ---- selection + Gauss-Newton refinement -------------------------------------------------------------------------------

constexpr int NV = 29;   // 21 (upper triangle of J^T J) + 6 (J^T r) + cost + inliers

// Sum over the block in a fixed order: xor butterfly in each wave, then the four wave partials in wave order.  `red` holds
// [4][nv] doubles, `out` receives nv sums; every thread returns after `out` is valid.
template <int N>
__device__ void block_sum(double (&v)[N], double* red, double* out) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double x = v[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    if (lane == 0) red[wv * N + i] = x;
  }
  __syncthreads();
  if (tid < N) out[tid] = (red[0 * N + tid] + red[1 * N + tid]) + (red[2 * N + tid] + red[3 * N + tid]);
  __syncthreads();
}

__device__ __forceinline__ void to_camera(const double* R, const double* t, const double* X, double* xc) {
  for (int r = 0; r < 3; ++r) xc[r] = (R[r * 3 + 0] * X[0] + R[r * 3 + 1] * X[1] + R[r * 3 + 2] * X[2]) + t[r];
}

__device__ __forceinline__ bool inlier_of(const PnPArgs& a, const double* R, const double* t, const double* X,
                                          const double* px, double thr2) {
  double xc[3];
  to_camera(R, t, X, xc);
  if (!(xc[2] > 0.0)) return false;
  const double ex = a.fx * xc[0] / xc[2] - (px[0] - a.u), ey = a.fy * xc[1] / xc[2] - (px[1] - a.v);
  return ex * ex + ey * ey < thr2;
}

// grid (B); dynamic LDS: the uint16 candidate list
__global__ __launch_bounds__(NT) void pnp_refine_kernel(PnPArgs a, const float* __restrict__ hp,
                                                        const int* __restrict__ counts, float* __restrict__ poses,
                                                        int* __restrict__ info) {
  extern __shared__ unsigned short list[];
  __shared__ int wave_tot[NT / 64];
  __shared__ int best_c[NT / 64], best_k[NT / 64];
  __shared__ double red[4 * NV];
  __shared__ double sums[NV];
  __shared__ double pose[12], cand[12];   // R row-major, t
  __shared__ int stop;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int b = blockIdx.x;
  const float* r = a.rec + (size_t)b * a.h * a.w * a.ld;
  const int n = build_candidates(a, r, list, wave_tot);
  const double fx = a.fx, fy = a.fy, thr2 = (double)a.thr * (double)a.thr;

  // selection: most inliers, ties to the lowest index
  int bc = -1, bk = -1;
  for (int k = tid; k < a.H; k += NT) {
    const int c = counts[(size_t)b * a.H + k];
    if (c > bc) { bc = c; bk = k; }            // k ascends: a later equal count never wins
  }
  for (int o = 32; o > 0; o >>= 1) {
    const int oc = __shfl_xor(bc, o), ok = __shfl_xor(bk, o);
    if (oc > bc || (oc == bc && ok >= 0 && (bk < 0 || ok < bk))) { bc = oc; bk = ok; }
  }
  if (lane == 0) { best_c[wv] = bc; best_k[wv] = bk; }
  __syncthreads();
  if (tid == 0) {
    int c = best_c[0], k = best_k[0];
    for (int w = 1; w < NT / 64; ++w)
      if (best_c[w] > c || (best_c[w] == c && best_k[w] >= 0 && (k < 0 || best_k[w] < k))) { c = best_c[w]; k = best_k[w]; }
    best_c[0] = c;
    best_k[0] = k;
  }
  __syncthreads();
  const int best = best_k[0], best_count = best_c[0];
  const int status = n < a.min_points ? KFN_PNP_TOO_FEW_POINTS : (best_count < 0 ? KFN_PNP_NO_HYPOTHESIS : KFN_PNP_OK);
  if (status != KFN_PNP_OK) {
    if (tid < 16) poses[(size_t)b * 16 + tid] = __builtin_nanf("");
    if (tid == 0) {
      info[b * 4 + 0] = status; info[b * 4 + 1] = n; info[b * 4 + 2] = 0; info[b * 4 + 3] = -1;
    }
    return;
  }
  if (tid < 12) {
    const float* o = hp + ((size_t)b * a.H + best) * 12;
    pose[tid] = (double)o[(tid < 9) ? (tid / 3) * 4 + tid % 3 : (tid - 9) * 4 + 3];
  }
  if (tid == 0) stop = 0;
  __syncthreads();

  for (int it = 0; it < a.iters; ++it) {
    // normal equations over the inliers of the current pose
    double acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0.0;
    for (int j = tid; j < n; j += NT) {
      double X[3], px[2], xc[3];
      load_point(a, r, list[j], X, px);
      to_camera(pose, pose + 9, X, xc);
      if (!(xc[2] > 0.0)) continue;
      const double iz = 1.0 / xc[2];
      const double ru = fx * xc[0] * iz - (px[0] - a.u), rv = fy * xc[1] * iz - (px[1] - a.v);
      if (!(ru * ru + rv * rv < thr2)) continue;
      const double a0 = fx * iz, a2 = -fx * xc[0] * iz * iz, b1 = fy * iz, b2 = -fy * xc[1] * iz * iz;
      const double Ju[6] = {a2 * xc[1], a0 * xc[2] - a2 * xc[0], -a0 * xc[1], a0, 0.0, a2};
      const double Jv[6] = {-b1 * xc[2] + b2 * xc[1], -b2 * xc[0], b1 * xc[0], 0.0, b1, b2};
      int q = 0;
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int k = i; k < 6; ++k) acc[q++] += Ju[i] * Ju[k] + Jv[i] * Jv[k];
#pragma unroll
      for (int i = 0; i < 6; ++i) acc[21 + i] += Ju[i] * ru + Jv[i] * rv;
      acc[27] += ru * ru + rv * rv;
      acc[28] += 1.0;
    }
    block_sum(acc, red, sums);
    if (tid == 0) {
      // Cholesky of the 6x6 system, solve H d = -g, candidate pose exp(w) R, exp(w) t + tau
      double L[6][6], g[6], d[6];
      int q = 0;
      for (int i = 0; i < 6; ++i)
        for (int k = i; k < 6; ++k) { L[k][i] = sums[q]; L[i][k] = sums[q]; ++q; }
      for (int i = 0; i < 6; ++i) g[i] = sums[21 + i];
      bool pd = sums[28] >= 3.0;
      for (int j = 0; j < 6 && pd; ++j) {
        double s = L[j][j];
        for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
        if (!(s > 0.0)) { pd = false; break; }
        L[j][j] = sqrt(s);
        for (int i = j + 1; i < 6; ++i) {
          double t = L[i][j];
          for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
          L[i][j] = t / L[j][j];
        }
      }
      if (!pd) {
        stop = 1;
      } else {
        double y[6];
        for (int i = 0; i < 6; ++i) {
          double s = -g[i];
          for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
          y[i] = s / L[i][i];
        }
        for (int i = 5; i >= 0; --i) {
          double s = y[i];
          for (int k = i + 1; k < 6; ++k) s -= L[k][i] * d[k];
          d[i] = s / L[i][i];
        }
        const double th = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        const double K[9] = {0.0, -d[2], d[1], d[2], 0.0, -d[0], -d[1], d[0], 0.0};
        double KK[9], E[9];
        for (int rr = 0; rr < 3; ++rr)
          for (int c = 0; c < 3; ++c)
            KK[rr * 3 + c] = K[rr * 3 + 0] * K[0 * 3 + c] + K[rr * 3 + 1] * K[1 * 3 + c] + K[rr * 3 + 2] * K[2 * 3 + c];
        const double s1 = th < 1e-12 ? 1.0 : sin(th) / th;
        const double s2 = th < 1e-12 ? 0.0 : (1.0 - cos(th)) / (th * th);
        for (int i = 0; i < 9; ++i) E[i] = ((i % 4 == 0) ? 1.0 : 0.0) + s1 * K[i] + s2 * KK[i];
        for (int rr = 0; rr < 3; ++rr) {
          for (int c = 0; c < 3; ++c)
            cand[rr * 3 + c] = E[rr * 3 + 0] * pose[0 * 3 + c] + E[rr * 3 + 1] * pose[1 * 3 + c] + E[rr * 3 + 2] * pose[2 * 3 + c];
          cand[9 + rr] = (E[rr * 3 + 0] * pose[9] + E[rr * 3 + 1] * pose[10] + E[rr * 3 + 2] * pose[11]) + d[3 + rr];
        }
      }
    }
    __syncthreads();
    if (stop) break;
    // cost of the candidate over the same inlier set
    double c2[2] = {0.0, 0.0};   // cost, points behind the camera
    for (int j = tid; j < n; j += NT) {
      double X[3], px[2], xc[3];
      load_point(a, r, list[j], X, px);
      if (!inlier_of(a, pose, pose + 9, X, px, thr2)) continue;
      to_camera(cand, cand + 9, X, xc);
      if (!(xc[2] > 0.0)) { c2[1] += 1.0; continue; }
      const double ru = fx * xc[0] / xc[2] - (px[0] - a.u), rv = fy * xc[1] / xc[2] - (px[1] - a.v);
      c2[0] += ru * ru + rv * rv;
    }
    block_sum(c2, red, sums + 21);   // (sums[21..22]: g is no longer needed; sums[27] still holds the cost)
    if (tid == 0) {
      if (sums[22] == 0.0 && sums[21] < sums[27]) {
        for (int i = 0; i < 12; ++i) pose[i] = cand[i];
      } else {
        stop = 1;
      }
    }
    __syncthreads();
    if (stop) break;
  }

  // final inliers; camera-to-world [R^T | -R^T t]
  double ni[1] = {0.0};
  for (int j = tid; j < n; j += NT) {
    double X[3], px[2];
    load_point(a, r, list[j], X, px);
    ni[0] += inlier_of(a, pose, pose + 9, X, px, thr2) ? 1.0 : 0.0;
  }
  block_sum(ni, red, sums);
  if (tid < 16) {
    const int rr = tid / 4, c = tid % 4;
    double val;
    if (rr == 3) val = (c == 3) ? 1.0 : 0.0;
    else if (c < 3) val = pose[c * 3 + rr];
    else val = -(pose[0 * 3 + rr] * pose[9] + pose[1 * 3 + rr] * pose[10] + pose[2 * 3 + rr] * pose[11]);
    poses[(size_t)b * 16 + tid] = (float)val;
  }
  if (tid == 0) {
    info[b * 4 + 0] = KFN_PNP_OK; info[b * 4 + 1] = n; info[b * 4 + 2] = (int)sums[0]; info[b * 4 + 3] = best;
  }
}

// ---- uncertainty (kfn_pnp_ransac_unc): the records' sigma propagated to the image plane ---------------------------------
// S = sigma^2 A A^T + pixel_sigma^2 I with A = d(pixel)/d(camera point) at xc; W = S^-1 by the closed form of the symmetric
// 2x2 inverse.  sig2 = sigma^2 = 1 / record[3]^2, ps2 = pixel_sigma^2.
struct Weight2 { double w00, w01, w11; };

__device__ __forceinline__ Weight2 measurement_weight(double fx, double fy, const double* xc, double sig2, double ps2) {
  const double iz = 1.0 / xc[2];
  const double a0 = fx * iz, a2 = -fx * xc[0] * iz * iz, b1 = fy * iz, b2 = -fy * xc[1] * iz * iz;
  const double s00 = sig2 * (a0 * a0 + a2 * a2) + ps2, s01 = sig2 * (a2 * b2), s11 = sig2 * (b1 * b1 + b2 * b2) + ps2;
  const double id = 1.0 / (s00 * s11 - s01 * s01);
  return Weight2{s11 * id, -s01 * id, s00 * id};
}

__device__ __forceinline__ double sigma2_of(const PnPArgs& a, const float* r, int cell) {
  const double c = (double)r[(size_t)cell * a.ld + 3];
  return 1.0 / (c * c);
}

// One inlier's terms of the weighted normal equations at `pose` (Z > 0 there: the caller's inlier test):
// acc[0..20] += upper triangle of J^T W J, acc[21..26] += J^T W r, acc[27] += r^T W r, acc[28] += 1.
__device__ __forceinline__ void weighted_terms(const PnPArgs& a, const double* pose, const double* X, const double* px,
                                               double sig2, double ps2, double* acc) {
  const double fx = a.fx, fy = a.fy;
  double xc[3];
  to_camera(pose, pose + 9, X, xc);
  const double iz = 1.0 / xc[2];
  const double ru = fx * xc[0] * iz - (px[0] - a.u), rv = fy * xc[1] * iz - (px[1] - a.v);
  const double a0 = fx * iz, a2 = -fx * xc[0] * iz * iz, b1 = fy * iz, b2 = -fy * xc[1] * iz * iz;
  const double Ju[6] = {a2 * xc[1], a0 * xc[2] - a2 * xc[0], -a0 * xc[1], a0, 0.0, a2};
  const double Jv[6] = {-b1 * xc[2] + b2 * xc[1], -b2 * xc[0], b1 * xc[0], 0.0, b1, b2};
  const Weight2 W = measurement_weight(fx, fy, xc, sig2, ps2);
  double Wu[6], Wv[6];   // rows of W J
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    Wu[i] = W.w00 * Ju[i] + W.w01 * Jv[i];
    Wv[i] = W.w01 * Ju[i] + W.w11 * Jv[i];
  }
  int q = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int k = i; k < 6; ++k) acc[q++] += Wu[i] * Ju[k] + Wv[i] * Jv[k];
#pragma unroll
  for (int i = 0; i < 6; ++i) acc[21 + i] += Wu[i] * ru + Wv[i] * rv;
  acc[27] += (W.w00 * ru * ru + 2.0 * W.w01 * ru * rv) + W.w11 * rv * rv;
  acc[28] += 1.0;
}

// Sigma = H^-1 from the Cholesky factor of the 6x6 H whose upper triangle is h[0..20] (row by row): L^-1 by forward
// substitution, Sigma = L^-T L^-1 with the upper triangle computed and mirrored, so Sigma is symmetric to the last bit.
// Returns false (Sigma untouched) if H is not positive definite.
__device__ bool inverse_spd6(const double* h, double (*Sg)[6]) {
  double L[6][6], Li[6][6];
  int q = 0;
  for (int i = 0; i < 6; ++i)
    for (int k = i; k < 6; ++k) { L[k][i] = h[q]; L[i][k] = h[q]; ++q; }
  for (int j = 0; j < 6; ++j) {
    double s = L[j][j];
    for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
    if (!(s > 0.0)) return false;
    L[j][j] = sqrt(s);
    for (int i = j + 1; i < 6; ++i) {
      double t = L[i][j];
      for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
      L[i][j] = t / L[j][j];
    }
  }
  for (int j = 0; j < 6; ++j) {
    Li[j][j] = 1.0 / L[j][j];
    for (int i = j + 1; i < 6; ++i) {
      double s = 0.0;
      for (int k = j; k < i; ++k) s -= L[i][k] * Li[k][j];
      Li[i][j] = s / L[i][i];
    }
  }
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) {
      double s = 0.0;
      for (int k = j; k < 6; ++k) s += Li[k][i] * Li[k][j];
      Sg[i][j] = s;
      Sg[j][i] = s;
    }
  return true;
}

// pnp_refine_kernel's sibling behind kfn_pnp_ransac_unc: the same grid, LDS, selection and loop; it also writes cov [B,36]
// and quality [B,2] (either may be null), and WEIGHTED weighs every inlier's residual by S^-1 (above) in the normal
// equations and in both costs.  <false> repeats pnp_refine_kernel's arithmetic statement for statement: the same bits in
// poses and info.  A sibling, not a template over both: pnp_refine_kernel is left as it was compiled before.
template <bool WEIGHTED>
__global__ __launch_bounds__(NT) void pnp_refine_unc_kernel(PnPArgs a, double ps2, const float* __restrict__ hp,
                                                            const int* __restrict__ counts, float* __restrict__ poses,
                                                            float* __restrict__ cov, float* __restrict__ quality,
                                                            int* __restrict__ info) {
  extern __shared__ unsigned short list[];
  __shared__ int wave_tot[NT / 64];
  __shared__ int best_c[NT / 64], best_k[NT / 64];
  __shared__ double red[4 * NV];
  __shared__ double sums[NV];
  __shared__ double pose[12], cand[12];   // R row-major, t
  __shared__ int stop;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int b = blockIdx.x;
  const float* r = a.rec + (size_t)b * a.h * a.w * a.ld;
  const int n = build_candidates(a, r, list, wave_tot);
  const double fx = a.fx, fy = a.fy, thr2 = (double)a.thr * (double)a.thr;

  // selection: most inliers, ties to the lowest index
  int bc = -1, bk = -1;
  for (int k = tid; k < a.H; k += NT) {
    const int c = counts[(size_t)b * a.H + k];
    if (c > bc) { bc = c; bk = k; }            // k ascends: a later equal count never wins
  }
  for (int o = 32; o > 0; o >>= 1) {
    const int oc = __shfl_xor(bc, o), ok = __shfl_xor(bk, o);
    if (oc > bc || (oc == bc && ok >= 0 && (bk < 0 || ok < bk))) { bc = oc; bk = ok; }
  }
  if (lane == 0) { best_c[wv] = bc; best_k[wv] = bk; }
  __syncthreads();
  if (tid == 0) {
    int c = best_c[0], k = best_k[0];
    for (int w = 1; w < NT / 64; ++w)
      if (best_c[w] > c || (best_c[w] == c && best_k[w] >= 0 && (k < 0 || best_k[w] < k))) { c = best_c[w]; k = best_k[w]; }
    best_c[0] = c;
    best_k[0] = k;
  }
  __syncthreads();
  const int best = best_k[0], best_count = best_c[0];
  const int status = n < a.min_points ? KFN_PNP_TOO_FEW_POINTS : (best_count < 0 ? KFN_PNP_NO_HYPOTHESIS : KFN_PNP_OK);
  if (status != KFN_PNP_OK) {
    if (tid < 16) poses[(size_t)b * 16 + tid] = __builtin_nanf("");
    if (tid == 0) {
      info[b * 4 + 0] = status; info[b * 4 + 1] = n; info[b * 4 + 2] = 0; info[b * 4 + 3] = -1;
    }
    if (cov && tid < 36) cov[(size_t)b * 36 + tid] = __builtin_nanf("");
    if (quality && tid < 2) quality[(size_t)b * 2 + tid] = __builtin_nanf("");
    return;
  }
  if (tid < 12) {
    const float* o = hp + ((size_t)b * a.H + best) * 12;
    pose[tid] = (double)o[(tid < 9) ? (tid / 3) * 4 + tid % 3 : (tid - 9) * 4 + 3];
  }
  if (tid == 0) stop = 0;
  __syncthreads();

  for (int it = 0; it < a.iters; ++it) {
    // normal equations over the inliers of the current pose
    double acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0.0;
    for (int j = tid; j < n; j += NT) {
      double X[3], px[2], xc[3];
      load_point(a, r, list[j], X, px);
      to_camera(pose, pose + 9, X, xc);
      if (!(xc[2] > 0.0)) continue;
      const double iz = 1.0 / xc[2];
      const double ru = fx * xc[0] * iz - (px[0] - a.u), rv = fy * xc[1] * iz - (px[1] - a.v);
      if (!(ru * ru + rv * rv < thr2)) continue;
      if constexpr (WEIGHTED) {
        weighted_terms(a, pose, X, px, sigma2_of(a, r, list[j]), ps2, acc);
        continue;
      }
      const double a0 = fx * iz, a2 = -fx * xc[0] * iz * iz, b1 = fy * iz, b2 = -fy * xc[1] * iz * iz;
      const double Ju[6] = {a2 * xc[1], a0 * xc[2] - a2 * xc[0], -a0 * xc[1], a0, 0.0, a2};
      const double Jv[6] = {-b1 * xc[2] + b2 * xc[1], -b2 * xc[0], b1 * xc[0], 0.0, b1, b2};
      int q = 0;
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int k = i; k < 6; ++k) acc[q++] += Ju[i] * Ju[k] + Jv[i] * Jv[k];
#pragma unroll
      for (int i = 0; i < 6; ++i) acc[21 + i] += Ju[i] * ru + Jv[i] * rv;
      acc[27] += ru * ru + rv * rv;
      acc[28] += 1.0;
    }
    block_sum(acc, red, sums);
    if (tid == 0) {
      // Cholesky of the 6x6 system, solve H d = -g, candidate pose exp(w) R, exp(w) t + tau
      double L[6][6], g[6], d[6];
      int q = 0;
      for (int i = 0; i < 6; ++i)
        for (int k = i; k < 6; ++k) { L[k][i] = sums[q]; L[i][k] = sums[q]; ++q; }
      for (int i = 0; i < 6; ++i) g[i] = sums[21 + i];
      bool pd = sums[28] >= 3.0;
      for (int j = 0; j < 6 && pd; ++j) {
        double s = L[j][j];
        for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
        if (!(s > 0.0)) { pd = false; break; }
        L[j][j] = sqrt(s);
        for (int i = j + 1; i < 6; ++i) {
          double t = L[i][j];
          for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
          L[i][j] = t / L[j][j];
        }
      }
      if (!pd) {
        stop = 1;
      } else {
        double y[6];
        for (int i = 0; i < 6; ++i) {
          double s = -g[i];
          for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
          y[i] = s / L[i][i];
        }
        for (int i = 5; i >= 0; --i) {
          double s = y[i];
          for (int k = i + 1; k < 6; ++k) s -= L[k][i] * d[k];
          d[i] = s / L[i][i];
        }
        const double th = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        const double K[9] = {0.0, -d[2], d[1], d[2], 0.0, -d[0], -d[1], d[0], 0.0};
        double KK[9], E[9];
        for (int rr = 0; rr < 3; ++rr)
          for (int c = 0; c < 3; ++c)
            KK[rr * 3 + c] = K[rr * 3 + 0] * K[0 * 3 + c] + K[rr * 3 + 1] * K[1 * 3 + c] + K[rr * 3 + 2] * K[2 * 3 + c];
        const double s1 = th < 1e-12 ? 1.0 : sin(th) / th;
        const double s2 = th < 1e-12 ? 0.0 : (1.0 - cos(th)) / (th * th);
        for (int i = 0; i < 9; ++i) E[i] = ((i % 4 == 0) ? 1.0 : 0.0) + s1 * K[i] + s2 * KK[i];
        for (int rr = 0; rr < 3; ++rr) {
          for (int c = 0; c < 3; ++c)
            cand[rr * 3 + c] = E[rr * 3 + 0] * pose[0 * 3 + c] + E[rr * 3 + 1] * pose[1 * 3 + c] + E[rr * 3 + 2] * pose[2 * 3 + c];
          cand[9 + rr] = (E[rr * 3 + 0] * pose[9] + E[rr * 3 + 1] * pose[10] + E[rr * 3 + 2] * pose[11]) + d[3 + rr];
        }
      }
    }
    __syncthreads();
    if (stop) break;
    // cost of the candidate over the same inlier set
    double c2[2] = {0.0, 0.0};   // cost, points behind the camera
    for (int j = tid; j < n; j += NT) {
      double X[3], px[2], xc[3];
      load_point(a, r, list[j], X, px);
      if (!inlier_of(a, pose, pose + 9, X, px, thr2)) continue;
      to_camera(cand, cand + 9, X, xc);
      if (!(xc[2] > 0.0)) { c2[1] += 1.0; continue; }
      const double ru = fx * xc[0] / xc[2] - (px[0] - a.u), rv = fy * xc[1] / xc[2] - (px[1] - a.v);
      if constexpr (WEIGHTED) {   // S stays the one of the current pose
        double xp[3];
        to_camera(pose, pose + 9, X, xp);
        const Weight2 W = measurement_weight(fx, fy, xp, sigma2_of(a, r, list[j]), ps2);
        c2[0] += (W.w00 * ru * ru + 2.0 * W.w01 * ru * rv) + W.w11 * rv * rv;
        continue;
      }
      c2[0] += ru * ru + rv * rv;
    }
    block_sum(c2, red, sums + 21);   // (sums[21..22]: g is no longer needed; sums[27] still holds the cost)
    if (tid == 0) {
      if (sums[22] == 0.0 && sums[21] < sums[27]) {
        for (int i = 0; i < 12; ++i) pose[i] = cand[i];
      } else {
        stop = 1;
      }
    }
    __syncthreads();
    if (stop) break;
  }

  // final inliers (pnp_refine_kernel's count, by its rule) and their weighted normal equations at the final pose:
  // Sigma = H^-1, quality = (cost, 2 * inliers - 6); camera-to-world [R^T | -R^T t]
  double acc[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) acc[i] = 0.0;
  for (int j = tid; j < n; j += NT) {
    double X[3], px[2];
    load_point(a, r, list[j], X, px);
    if (inlier_of(a, pose, pose + 9, X, px, thr2)) weighted_terms(a, pose, X, px, sigma2_of(a, r, list[j]), ps2, acc);
  }
  block_sum(acc, red, sums);
  const int inliers = (int)sums[28];
  if (tid == 0) {
    double Sg[6][6];
    const bool pd = inliers >= 3 && inverse_spd6(sums, Sg);
    if (cov)
      for (int i = 0; i < 36; ++i) cov[(size_t)b * 36 + i] = pd ? (float)Sg[i / 6][i % 6] : __builtin_nanf("");
    if (quality) {
      quality[(size_t)b * 2 + 0] = (float)sums[27];
      quality[(size_t)b * 2 + 1] = (float)(2 * inliers - 6);
    }
  }
  if (tid < 16) {
    const int rr = tid / 4, c = tid % 4;
    double val;
    if (rr == 3) val = (c == 3) ? 1.0 : 0.0;
    else if (c < 3) val = pose[c * 3 + rr];
    else val = -(pose[0 * 3 + rr] * pose[9] + pose[1 * 3 + rr] * pose[10] + pose[2 * 3 + rr] * pose[11]);
    poses[(size_t)b * 16 + tid] = (float)val;
  }
  if (tid == 0) {
    info[b * 4 + 0] = KFN_PNP_OK; info[b * 4 + 1] = n; info[b * 4 + 2] = inliers; info[b * 4 + 3] = best;
  }
}

// ---- guided sampling (kfn_pnp_ransac_guided): draws in proportion to the confidence above the threshold ----------------
// DESIGN.md 5c "Guided sampling" and tests/pnp_guided_ref.py state the same rule.  A candidate's integer weight, from
// c = record[3] in binary32, every operation rounded to nearest (a subtraction feeds a multiplication by a power of two: no
// contraction applies): q = (int)floorf((fminf(c, cap) - minc) * 16) + 1 >= 1; w = q, or q * q in the squared mode.
// With cap <= 4096, q <= 65537 and the sum of 32768 weights stays below 2^48.
__device__ __forceinline__ unsigned long long guided_weight(float c, float minc, float cap, int squared) {
  const float d = fminf(c, cap) - minc;
  const unsigned long long q = (unsigned long long)((int)floorf(d * 16.0f) + 1);
  return squared ? q * q : q;
}

// grid (B): cum[b][i] = w[0] + .. + w[i] over the frame's candidates in raster order (build_candidates' order and rule),
// ncand[b] = n.  An order-preserving block scan in uint64: a ballot prefix places a candidate, a shuffle prefix sums the
// weights within a wave, the wave totals are added in wave order and a carry runs from chunk to chunk.
__global__ __launch_bounds__(NT) void pnp_cdf_kernel(PnPArgs a, float cap, int squared, unsigned long long* __restrict__ cum,
                                                     int* __restrict__ ncand) {
  __shared__ int wave_tot[NT / 64];
  __shared__ unsigned long long wave_sum[NT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int b = blockIdx.x;
  const int hw = a.h * a.w;
  const float* r = a.rec + (size_t)b * hw * a.ld;
  unsigned long long* out = cum + (size_t)b * hw;
  int base = 0;
  unsigned long long carry = 0;
  for (int c0 = 0; c0 < hw; c0 += NT) {
    const int c = c0 + tid;
    const bool keep = c < hw && is_candidate(r + (size_t)c * a.ld, a.minc);
    unsigned long long x = keep ? guided_weight(r[(size_t)c * a.ld + 3], a.minc, cap, squared) : 0ull;
    const unsigned long long m = __ballot(keep);
    const int pre = __popcll(m & ((1ull << lane) - 1ull));
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long y = __shfl_up(x, o);
      if (lane >= o) x += y;
    }
    if (lane == 63) { wave_tot[wv] = __popcll(m); wave_sum[wv] = x; }
    __syncthreads();
    int off = base;
    unsigned long long s = carry;
    for (int k = 0; k < wv; ++k) { off += wave_tot[k]; s += wave_sum[k]; }
    if (keep) out[off + pre] = s + x;
    base += (wave_tot[0] + wave_tot[1]) + (wave_tot[2] + wave_tot[3]);
    carry += (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
    __syncthreads();
  }
  if (tid == 0) ncand[b] = base;
}

// pnp_hyp_kernel's sibling behind kfn_pnp_ransac_guided: the same grid, candidate list, hash, P3P and outputs; the index of
// a draw is the first i with cum[i] > floor(hash * total / 2^32), found by bisection in the frame's row of `cum`.  A
// sibling, not a template over both: pnp_hyp_kernel is left as it was compiled before.
__global__ __launch_bounds__(NT) void pnp_hyp_guided_kernel(PnPArgs a, const unsigned long long* __restrict__ cum,
                                                            int* __restrict__ samples, float* __restrict__ hp,
                                                            int* __restrict__ counts) {
  extern __shared__ unsigned short list[];
  __shared__ int wave_tot[NT / 64];
  const int b = blockIdx.y;
  const int k = blockIdx.x * NT + threadIdx.x;
  const float* r = a.rec + (size_t)b * a.h * a.w * a.ld;
  const unsigned long long* cf = cum + (size_t)b * a.h * a.w;
  const int n = build_candidates(a, r, list, wave_tot);
  if (k >= a.H) return;
  int s[4] = {-1, -1, -1, -1};
  int got = 0;
  if (n >= a.min_points) {
    const unsigned long long total = cf[n - 1];
    const uint32_t frame = (uint32_t)(a.t0 + b);
    const uint32_t key = a.seed ^ (frame * 0x9E3779B1u) ^ ((uint32_t)k * 0x85EBCA77u);
    for (int draw = 0; draw < MAX_DRAWS && got < 4; ++draw) {
      const unsigned long long hsh = lowbias32(key ^ ((uint32_t)draw * 0xC2B2AE3Du));
      // the 96-bit product's bits 32..95 (bits 80.. are 0: hsh < 2^32, total < 2^48); target < total = cum[n - 1]
      const unsigned long long target = (__umul64hi(hsh, total) << 32) | ((hsh * total) >> 32);
      int lo = 0, hi = n - 1;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cf[mid] > target) hi = mid; else lo = mid + 1;
      }
      const int idx = lo;
      bool dup = false;
      for (int i = 0; i < got; ++i) dup |= s[i] == idx;
      if (!dup) s[got++] = idx;
    }
  }
  const bool sampled = got == 4;
  const size_t hk = (size_t)b * a.H + k;
  if (samples)
    for (int i = 0; i < 4; ++i) samples[hk * 4 + i] = sampled ? s[i] : -1;
  double R[9], t[3];
  bool ok = false;
  if (sampled) {
    double X[4][3], px[4][2];
    for (int i = 0; i < 4; ++i) load_point(a, r, list[s[i]], X[i], px[i]);
    ok = p3p_hypothesis(a, X, px, R, t);
  }
  float* o = hp + hk * 12;
  for (int rr = 0; rr < 3; ++rr) {
    for (int c = 0; c < 3; ++c) o[rr * 4 + c] = ok ? (float)R[rr * 3 + c] : __builtin_nanf("");
    o[rr * 4 + 3] = ok ? (float)t[rr] : __builtin_nanf("");
  }
  counts[hk] = ok ? 0 : -1;
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Copy of the caller's descriptor (struct_size bytes, the rest 0) and the argument checks shared by the entry points.
int pnp_desc_in(const kfn_pnp_desc* in, kfn_pnp_desc* d, const char* who) {
  if (in == nullptr) return kfn::fail(KFN_ERR_ARG, "%s: null descriptor", who);
  const int32_t sz = in->struct_size;
  if (sz < (int32_t)sizeof(kfn_pnp_desc) || (sz & 3) != 0)     // the ABI-11 struct is the smallest there is
    return kfn::fail(KFN_ERR_ARG, "%s: kfn_pnp_desc.struct_size = %d (this library: %d bytes) -- use KFN_PNP_DESC_INIT", who,
                     (int)sz, (int)sizeof(kfn_pnp_desc));
  std::memset(d, 0, sizeof(*d));
  std::memcpy(d, in, sizeof(*d));   // (a larger struct from a newer host: its tail is not read)
  KFN_REQUIRE(d->B > 0 && d->h > 0 && d->w > 0, "%s: bad shape B=%d h=%d w=%d", who, d->B, d->h, d->w);
  KFN_REQUIRE((long)d->h * d->w <= MAX_CELLS, "%s: h*w = %ld cells, at most %d", who, (long)d->h * d->w, MAX_CELLS);
  KFN_REQUIRE(d->ld >= 4, "%s: ld = %d < 4", who, d->ld);
  KFN_REQUIRE(d->t0 >= 0, "%s: t0 = %d < 0", who, d->t0);
  KFN_REQUIRE(d->hypotheses >= 1 && d->hypotheses <= KFN_PNP_MAX_HYPOTHESES, "%s: hypotheses = %d (1..%d)", who,
              d->hypotheses, KFN_PNP_MAX_HYPOTHESES);
  KFN_REQUIRE(d->refine_iters >= 0 && d->refine_iters <= 100, "%s: refine_iters = %d (0..100)", who, d->refine_iters);
  KFN_REQUIRE(d->min_points >= 4, "%s: min_points = %d < 4", who, d->min_points);
  KFN_REQUIRE(d->fx > 0.f && d->fy > 0.f && std::isfinite(d->fx) && std::isfinite(d->fy) && std::isfinite(d->u) &&
                  std::isfinite(d->v), "%s: bad intrinsics", who);
  KFN_REQUIRE(d->cell_stride > 0, "%s: cell_stride = %d", who, d->cell_stride);
  KFN_REQUIRE(d->inlier_px > 0.f && std::isfinite(d->inlier_px) && !std::isnan(d->min_confidence),
              "%s: bad inlier_px / min_confidence", who);
  return KFN_OK;
}

PnPArgs pnp_args(const kfn_pnp_desc* d, const float* records) {
  PnPArgs a;
  a.rec = records;
  a.B = d->B; a.h = d->h; a.w = d->w; a.ld = d->ld; a.t0 = d->t0;
  a.seed = d->seed;
  a.H = d->hypotheses; a.iters = d->refine_iters; a.min_points = d->min_points;
  a.fx = d->fx; a.fy = d->fy; a.u = d->u; a.v = d->v;
  a.cs = d->cell_stride;
  a.minc = d->min_confidence; a.thr = d->inlier_px;
  return a;
}

int launch_hyp_and_score(const PnPArgs& a, int* samples, float* hp, int* counts, hipStream_t st) {
  static std::atomic<uint64_t> hyp_lds_done{0}, ref_lds_done{0};
  const int list_bytes = 2 * a.h * a.w;
  int rc = kfn::set_max_dynamic_lds((const void*)pnp_hyp_kernel, 2 * MAX_CELLS, hyp_lds_done);
  if (rc == KFN_OK) rc = kfn::set_max_dynamic_lds((const void*)pnp_refine_kernel, 2 * MAX_CELLS, ref_lds_done);
  if (rc != KFN_OK) return rc;
  const unsigned hb = (unsigned)kfn::ceil_div(a.H, NT);
  hipLaunchKernelGGL(pnp_hyp_kernel, dim3(hb, (unsigned)a.B), dim3(NT), list_bytes, st, a, samples, hp, counts);
  KFN_LAUNCH_CHECK("pnp_hyp_kernel");
  hipLaunchKernelGGL(pnp_score_kernel, dim3((unsigned)kfn::ceil_div(a.h * a.w, TILE), hb, (unsigned)a.B), dim3(NT), 0, st, a,
                     (const float*)hp, counts);
  KFN_LAUNCH_CHECK("pnp_score_kernel");
  return KFN_OK;
}

}  // namespace

extern "C" int kfn_pnp_scratch_bytes(const kfn_pnp_desc* desc, size_t* bytes) {
  kfn_pnp_desc d;
  int rc = pnp_desc_in(desc, &d, "kfn_pnp_scratch_bytes");
  if (rc != KFN_OK) return rc;
  KFN_REQUIRE(bytes, "kfn_pnp_scratch_bytes: null bytes");
  const size_t bh = (size_t)d.B * d.hypotheses;
  *bytes = align256(bh * 12 * sizeof(float)) + align256(bh * sizeof(int32_t));
  return KFN_OK;
}

extern "C" int kfn_pnp_ransac(const kfn_pnp_desc* desc, const float* records, float* poses, int32_t* info, void* scratch,
                              void* stream) {
  kfn_pnp_desc d;
  int rc = pnp_desc_in(desc, &d, "kfn_pnp_ransac");
  if (rc != KFN_OK) return rc;
  KFN_REQUIRE(records && poses && info && scratch, "kfn_pnp_ransac: null argument");
  KFN_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 15) == 0, "kfn_pnp_ransac: scratch not 16-byte aligned");
  const PnPArgs a = pnp_args(&d, records);
  const size_t bh = (size_t)d.B * d.hypotheses;
  float* hp = static_cast<float*>(scratch);
  int* counts = reinterpret_cast<int*>(static_cast<char*>(scratch) + align256(bh * 12 * sizeof(float)));
  const hipStream_t st = (hipStream_t)stream;
  rc = launch_hyp_and_score(a, nullptr, hp, counts, st);
  if (rc != KFN_OK) return rc;
  hipLaunchKernelGGL(pnp_refine_kernel, dim3((unsigned)d.B), dim3(NT), 2 * d.h * d.w, st, a, (const float*)hp,
                     (const int*)counts, poses, info);
  KFN_LAUNCH_CHECK("pnp_refine_kernel");
  return KFN_OK;
}

extern "C" int kfn_pnp_ransac_unc(const kfn_pnp_desc* desc, const kfn_pnp_unc_desc* unc, const float* records, float* poses,
                                  float* cov, float* quality, int32_t* info, void* scratch, void* stream) {
  kfn_pnp_desc d;
  int rc = pnp_desc_in(desc, &d, "kfn_pnp_ransac_unc");
  if (rc != KFN_OK) return rc;
  if (unc == nullptr) return kfn::fail(KFN_ERR_ARG, "kfn_pnp_ransac_unc: null kfn_pnp_unc_desc");
  if (unc->struct_size < (int32_t)sizeof(kfn_pnp_unc_desc) || (unc->struct_size & 3) != 0)
    return kfn::fail(KFN_ERR_ARG, "kfn_pnp_ransac_unc: kfn_pnp_unc_desc.struct_size = %d (this library: %d bytes) -- use "
                     "KFN_PNP_UNC_DESC_INIT", (int)unc->struct_size, (int)sizeof(kfn_pnp_unc_desc));
  const kfn_pnp_unc_desc q = *unc;
  KFN_REQUIRE(q.weighted == 0 || q.weighted == 1, "kfn_pnp_ransac_unc: weighted = %d (0 or 1)", q.weighted);
  KFN_REQUIRE(q.pixel_sigma > 0.f && std::isfinite(q.pixel_sigma), "kfn_pnp_ransac_unc: pixel_sigma = %g, must be > 0",
              (double)q.pixel_sigma);
  KFN_REQUIRE(d.min_confidence >= 0.f, "kfn_pnp_ransac_unc: min_confidence = %g < 0 (sigma = 1 / confidence must be positive)",
              (double)d.min_confidence);
  KFN_REQUIRE(records && poses && info && scratch, "kfn_pnp_ransac_unc: null argument");
  KFN_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 15) == 0, "kfn_pnp_ransac_unc: scratch not 16-byte aligned");
  const PnPArgs a = pnp_args(&d, records);
  const size_t bh = (size_t)d.B * d.hypotheses;
  float* hp = static_cast<float*>(scratch);
  int* counts = reinterpret_cast<int*>(static_cast<char*>(scratch) + align256(bh * 12 * sizeof(float)));
  const hipStream_t st = (hipStream_t)stream;
  rc = launch_hyp_and_score(a, nullptr, hp, counts, st);
  if (rc != KFN_OK) return rc;
  static std::atomic<uint64_t> lds_done[2];
  const void* kernel = q.weighted ? (const void*)pnp_refine_unc_kernel<true> : (const void*)pnp_refine_unc_kernel<false>;
  rc = kfn::set_max_dynamic_lds(kernel, 2 * MAX_CELLS, lds_done[q.weighted]);
  if (rc != KFN_OK) return rc;
  const double ps2 = (double)q.pixel_sigma * (double)q.pixel_sigma;
  if (q.weighted)
    hipLaunchKernelGGL(pnp_refine_unc_kernel<true>, dim3((unsigned)d.B), dim3(NT), 2 * d.h * d.w, st, a, ps2, (const float*)hp,
                       (const int*)counts, poses, cov, quality, info);
  else
    hipLaunchKernelGGL(pnp_refine_unc_kernel<false>, dim3((unsigned)d.B), dim3(NT), 2 * d.h * d.w, st, a, ps2,
                       (const float*)hp, (const int*)counts, poses, cov, quality, info);
  KFN_LAUNCH_CHECK("pnp_refine_unc_kernel");
  return KFN_OK;
}

extern "C" int kfn_pnp_hypotheses(const kfn_pnp_desc* desc, const float* records, int32_t* samples, float* hyp_poses,
                                  int32_t* counts, void* stream) {
  kfn_pnp_desc d;
  int rc = pnp_desc_in(desc, &d, "kfn_pnp_hypotheses");
  if (rc != KFN_OK) return rc;
  KFN_REQUIRE(records && samples && hyp_poses && counts, "kfn_pnp_hypotheses: null argument");
  return launch_hyp_and_score(pnp_args(&d, records), samples, hyp_poses, counts, (hipStream_t)stream);
}

// ---- guided sampling: the entry points -----------------------------------------------------------------------------------

namespace {

// The checks on kfn_pnp_sample_desc shared by the guided entry points; `d` has passed pnp_desc_in.
int pnp_sample_in(const kfn_pnp_sample_desc* in, const kfn_pnp_desc& d, kfn_pnp_sample_desc* s, const char* who) {
  if (in == nullptr) return kfn::fail(KFN_ERR_ARG, "%s: null kfn_pnp_sample_desc", who);
  if (in->struct_size < (int32_t)sizeof(kfn_pnp_sample_desc) || (in->struct_size & 3) != 0)
    return kfn::fail(KFN_ERR_ARG, "%s: kfn_pnp_sample_desc.struct_size = %d (this library: %d bytes) -- use "
                     "KFN_PNP_SAMPLE_DESC_INIT", who, (int)in->struct_size, (int)sizeof(kfn_pnp_sample_desc));
  *s = *in;
  KFN_REQUIRE(s->mode == KFN_PNP_SAMPLE_CONFIDENCE || s->mode == KFN_PNP_SAMPLE_CONFIDENCE_SQ,
              "%s: mode = %d (KFN_PNP_SAMPLE_CONFIDENCE = 1 or KFN_PNP_SAMPLE_CONFIDENCE_SQ = 2)", who, s->mode);
  KFN_REQUIRE(d.min_confidence >= 0.f, "%s: min_confidence = %g < 0", who, (double)d.min_confidence);
  KFN_REQUIRE(std::isfinite(s->confidence_cap), "%s: confidence_cap = %g is not finite", who, (double)s->confidence_cap);
  KFN_REQUIRE(s->confidence_cap > d.min_confidence, "%s: confidence_cap = %g <= min_confidence = %g", who,
              (double)s->confidence_cap, (double)d.min_confidence);
  KFN_REQUIRE(s->confidence_cap <= 4096.f, "%s: confidence_cap = %g > 4096", who, (double)s->confidence_cap);
  return KFN_OK;
}

// The caller's scratch of a guided call: kfn_pnp_scratch_bytes' two arrays, then cum [B][h*w] uint64 and n [B].
struct GuidedScratch {
  float* hp;
  int* counts;
  unsigned long long* cum;
  int* ncand;
  size_t bytes;
};

GuidedScratch guided_scratch(const kfn_pnp_desc& d, void* scratch) {
  const size_t bh = (size_t)d.B * d.hypotheses, cells = (size_t)d.B * d.h * d.w;
  char* p = static_cast<char*>(scratch);
  GuidedScratch g;
  size_t off = 0;
  g.hp = reinterpret_cast<float*>(p + off);                off += align256(bh * 12 * sizeof(float));
  g.counts = reinterpret_cast<int*>(p + off);              off += align256(bh * sizeof(int32_t));
  g.cum = reinterpret_cast<unsigned long long*>(p + off);  off += align256(cells * sizeof(uint64_t));
  g.ncand = reinterpret_cast<int*>(p + off);               off += align256((size_t)d.B * sizeof(int32_t));
  g.bytes = off;
  return g;
}

int launch_guided_hyp_and_score(const PnPArgs& a, const kfn_pnp_sample_desc& s, unsigned long long* cum, int* ncand,
                                int* samples, float* hp, int* counts, hipStream_t st) {
  static std::atomic<uint64_t> hyp_lds_done{0};
  const int rc = kfn::set_max_dynamic_lds((const void*)pnp_hyp_guided_kernel, 2 * MAX_CELLS, hyp_lds_done);
  if (rc != KFN_OK) return rc;
  hipLaunchKernelGGL(pnp_cdf_kernel, dim3((unsigned)a.B), dim3(NT), 0, st, a, s.confidence_cap,
                     (int)(s.mode == KFN_PNP_SAMPLE_CONFIDENCE_SQ), cum, ncand);
  KFN_LAUNCH_CHECK("pnp_cdf_kernel");
  const unsigned hb = (unsigned)kfn::ceil_div(a.H, NT);
  hipLaunchKernelGGL(pnp_hyp_guided_kernel, dim3(hb, (unsigned)a.B), dim3(NT), 2 * a.h * a.w, st, a,
                     (const unsigned long long*)cum, samples, hp, counts);
  KFN_LAUNCH_CHECK("pnp_hyp_guided_kernel");
  hipLaunchKernelGGL(pnp_score_kernel, dim3((unsigned)kfn::ceil_div(a.h * a.w, TILE), hb, (unsigned)a.B), dim3(NT), 0, st, a,
                     (const float*)hp, counts);
  KFN_LAUNCH_CHECK("pnp_score_kernel");
  return KFN_OK;
}

}  // namespace

extern "C" int kfn_pnp_guided_scratch_bytes(const kfn_pnp_desc* desc, const kfn_pnp_sample_desc* sample, size_t* bytes) {
  kfn_pnp_desc d;
  kfn_pnp_sample_desc s;
  int rc = pnp_desc_in(desc, &d, "kfn_pnp_guided_scratch_bytes");
  if (rc == KFN_OK) rc = pnp_sample_in(sample, d, &s, "kfn_pnp_guided_scratch_bytes");
  if (rc != KFN_OK) return rc;
  KFN_REQUIRE(bytes, "kfn_pnp_guided_scratch_bytes: null bytes");
  *bytes = guided_scratch(d, nullptr).bytes;
  return KFN_OK;
}

extern "C" int kfn_pnp_ransac_guided(const kfn_pnp_desc* desc, const kfn_pnp_sample_desc* sample, const kfn_pnp_unc_desc* unc,
                                     const float* records, float* poses, float* cov, float* quality, int32_t* info,
                                     void* scratch, void* stream) {
  const char* who = "kfn_pnp_ransac_guided";
  kfn_pnp_desc d;
  kfn_pnp_sample_desc s;
  int rc = pnp_desc_in(desc, &d, who);
  if (rc == KFN_OK) rc = pnp_sample_in(sample, d, &s, who);
  if (rc != KFN_OK) return rc;
  kfn_pnp_unc_desc q = KFN_PNP_UNC_DESC_INIT;
  if (unc != nullptr) {
    if (unc->struct_size < (int32_t)sizeof(kfn_pnp_unc_desc) || (unc->struct_size & 3) != 0)
      return kfn::fail(KFN_ERR_ARG, "%s: kfn_pnp_unc_desc.struct_size = %d (this library: %d bytes) -- use "
                       "KFN_PNP_UNC_DESC_INIT", who, (int)unc->struct_size, (int)sizeof(kfn_pnp_unc_desc));
    q = *unc;
    KFN_REQUIRE(q.weighted == 0 || q.weighted == 1, "%s: weighted = %d (0 or 1)", who, q.weighted);
    KFN_REQUIRE(q.pixel_sigma > 0.f && std::isfinite(q.pixel_sigma), "%s: pixel_sigma = %g, must be > 0", who,
                (double)q.pixel_sigma);
  } else {
    KFN_REQUIRE(cov == nullptr && quality == nullptr, "%s: cov and quality need a kfn_pnp_unc_desc", who);
  }
  KFN_REQUIRE(records && poses && info && scratch, "%s: null argument", who);
  KFN_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 15) == 0, "%s: scratch not 16-byte aligned", who);
  const PnPArgs a = pnp_args(&d, records);
  const GuidedScratch g = guided_scratch(d, scratch);
  const hipStream_t st = (hipStream_t)stream;
  static std::atomic<uint64_t> lds_done[3];
  const void* kernel = unc == nullptr ? (const void*)pnp_refine_kernel
                       : (q.weighted ? (const void*)pnp_refine_unc_kernel<true> : (const void*)pnp_refine_unc_kernel<false>);
  rc = kfn::set_max_dynamic_lds(kernel, 2 * MAX_CELLS, lds_done[unc == nullptr ? 2 : q.weighted]);
  if (rc != KFN_OK) return rc;
  rc = launch_guided_hyp_and_score(a, s, g.cum, g.ncand, nullptr, g.hp, g.counts, st);
  if (rc != KFN_OK) return rc;
  const double ps2 = (double)q.pixel_sigma * (double)q.pixel_sigma;
  if (unc == nullptr)
    hipLaunchKernelGGL(pnp_refine_kernel, dim3((unsigned)d.B), dim3(NT), 2 * d.h * d.w, st, a, (const float*)g.hp,
                       (const int*)g.counts, poses, info);
  else if (q.weighted)
    hipLaunchKernelGGL(pnp_refine_unc_kernel<true>, dim3((unsigned)d.B), dim3(NT), 2 * d.h * d.w, st, a, ps2,
                       (const float*)g.hp, (const int*)g.counts, poses, cov, quality, info);
  else
    hipLaunchKernelGGL(pnp_refine_unc_kernel<false>, dim3((unsigned)d.B), dim3(NT), 2 * d.h * d.w, st, a, ps2,
                       (const float*)g.hp, (const int*)g.counts, poses, cov, quality, info);
  KFN_LAUNCH_CHECK(unc == nullptr ? "pnp_refine_kernel" : "pnp_refine_unc_kernel");
  return KFN_OK;
}

extern "C" int kfn_pnp_hypotheses_guided(const kfn_pnp_desc* desc, const kfn_pnp_sample_desc* sample, const float* records,
                                         int32_t* samples, float* hyp_poses, int32_t* counts, uint64_t* cum, int32_t* n,
                                         void* scratch, void* stream) {
  const char* who = "kfn_pnp_hypotheses_guided";
  kfn_pnp_desc d;
  kfn_pnp_sample_desc s;
  int rc = pnp_desc_in(desc, &d, who);
  if (rc == KFN_OK) rc = pnp_sample_in(sample, d, &s, who);
  if (rc != KFN_OK) return rc;
  KFN_REQUIRE(records && samples && hyp_poses && counts && scratch, "%s: null argument", who);
  KFN_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 15) == 0, "%s: scratch not 16-byte aligned", who);
  KFN_REQUIRE((reinterpret_cast<uintptr_t>(cum) & 7) == 0, "%s: cum not 8-byte aligned", who);
  const GuidedScratch g = guided_scratch(d, scratch);
  return launch_guided_hyp_and_score(pnp_args(&d, records), s, cum ? reinterpret_cast<unsigned long long*>(cum) : g.cum,
                                     n ? n : g.ncand, samples, hyp_poses, counts, (hipStream_t)stream);
}
