// kfn_kabsch.hip -- camera poses from the scene-coordinate records and a depth frame: batched RANSAC-Kabsch on the device.
//
// The sibling of kfn_pnp.hip for RGB-D input (DESIGN.md 5c "Poses with depth").  With the depth frame back-projected at the
// records' pixels (cam_points: kfn_depth_labels at stride 8 under the identity pose), every confident cell is a 3-D/3-D
// correspondence: camera point p, scene point x.  The pose is the rigid alignment x ~ R p + t, camera to world as it stands.
//   1. kabsch_hyp_kernel     one workgroup per (frame, 256 hypotheses): the frame's candidate list (raster order) in LDS, then
//                            one lane per hypothesis draws 3 distinct indices from kfn_pnp.hip's counter hash and solves the
//                            least-squares rigid transform of the three pairs in fp64 (Horn's quaternion form: the largest
//                            eigenvector of a symmetric 4x4, by cyclic Jacobi with a fixed number of sweeps); [R|t] in fp32.
//   2. kabsch_score_kernel   the hot path, pnp_score_kernel's decomposition: a grid of (cell tile, hypothesis block, frame); a
//                            tile's candidates compacted into LDS, six floats each; one hypothesis per lane in registers; the
//                            points read as broadcasts; inlier iff |R p + t - x|^2 < inlier_m^2 in fp32; the tile's integer
//                            count is added to the hypothesis' count with an integer atomic.
//   3. kabsch_refine_kernel  one workgroup per frame: the best hypothesis (ties to the lowest index), then up to refine_iters
//                            rounds of (inliers of the current pose, weighted closed form over them) in fp64, the 16 sums
//                            reduced in pnp_refine_kernel's fixed order; then the 6x6 covariance and (cost, 3 * inliers - 6).
// No host round trip between the stages, no device RNG state, no float atomics: the same bits on every launch.
#include <cmath>

#include "kfn_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int NT = 256;          // threads of every workgroup here; the hypothesis block of one lane per hypothesis
constexpr int TILE = 128;        // grid cells per scoring workgroup
constexpr int MAX_DRAWS = 16;
constexpr int MAX_CELLS = 32768; // the candidate list is uint16 cell indices in LDS: 64 KiB
constexpr int SWEEPS = 10;       // cyclic Jacobi on a symmetric 4x4: converged to the last bits after 6
constexpr double MIN_AREA2 = 1e-6;   // a triangle whose |(p1 - p0) x (p2 - p0)| is below this (m^2) gives no hypothesis
constexpr double MIN_GAP = 1e-9;     // the two largest eigenvalues closer than this share of the largest magnitude: degenerate

struct KabschArgs {
  const float* rec;
  const float* cam;
  int B, h, w, ld, ldp, t0;
  uint32_t seed;
  int H, iters, min_points;
  float minc, thr;
  int weighted;
  double ps2;      // point_sigma^2
};

__device__ __forceinline__ uint32_t lowbias32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// p: the record (x, y, z, 1/sigma), q: the camera point (Xc, Yc, Zc, mask)
__device__ __forceinline__ bool is_candidate(const float* p, const float* q, float minc) {
  return p[3] > minc && isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]) && q[3] == 1.0f && isfinite(q[0]) &&
         isfinite(q[1]) && isfinite(q[2]);
}

// The frame's candidates as cell indices in raster order (order-preserving: ballot prefix within a wave, wave totals in
// order).  Every thread of the 256-thread block takes part; returns n in every thread.
__device__ int build_candidates(const KabschArgs& a, const float* r, const float* cp, unsigned short* list, int* wave_tot) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int hw = a.h * a.w;
  int base = 0;
  for (int c0 = 0; c0 < hw; c0 += NT) {
    const int c = c0 + tid;
    const bool keep = c < hw && is_candidate(r + (size_t)c * a.ld, cp + (size_t)c * a.ldp, a.minc);
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

__device__ __forceinline__ void load_pair(const KabschArgs& a, const float* r, const float* cp, int cell, double* P, double* X) {
  const float* x = r + (size_t)cell * a.ld;
  const float* p = cp + (size_t)cell * a.ldp;
  P[0] = p[0]; P[1] = p[1]; P[2] = p[2];
  X[0] = x[0]; X[1] = x[1]; X[2] = x[2];
}

__device__ __forceinline__ double sigma2_of(const KabschArgs& a, const float* r, int cell) {
  const double c = (double)r[(size_t)cell * a.ld + 3];
  return 1.0 / (c * c);
}

// ---- the closed form: Horn's quaternion solution of the weighted rigid alignment, fp64 -----------------------------------

// Cyclic Jacobi on the symmetric 4x4 A (destroyed: its diagonal ends as the eigenvalues), V's columns the eigenvectors.
__device__ void jacobi4(double (*A)[4], double (*V)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) V[i][k] = i == k ? 1.0 : 0.0;
  for (int sweep = 0; sweep < SWEEPS; ++sweep) {
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        const double apq = A[p][q];
        if (apq == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
        const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq;
          A[k][q] = s * akp + c * akq;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk;
          A[q][k] = s * apk + c * aqk;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
  }
}

// s[16] = sum w, sum w p (3), sum w x (3), sum w p_a x_b (9, a major) -> the (R, t) that minimises sum w |R p + t - x|^2 with
// det R = +1; R row-major.  False (R, t untouched) when the sums are not finite, the weight is not positive or the rotation
// is not determined: the two largest eigenvalues of Horn's matrix within MIN_GAP of each other (points on one line).
// The gap rule is this project's addition to the triangle-area rule of a hypothesis: the refinement needs a test for a
// degenerate inlier set, one routine serves both, and so a long thin triangle whose area passes can still be refused here.
// S is formed from the uncentred sums, sum w p x^T - (sum w p) xbar^T: with coordinates of a few metres the subtraction
// costs the digits of (extent / distance from the origin)^2 -- about eight for millimetre edges at several metres, none
// that matter for the decimetre-and-up triangles and inlier sets the stage works on (fp64 leaves 1e-16 * 10 m^2 absolute).
__device__ bool kabsch_from_sums(const double* s, double* R, double* t) {
  const double W = s[0];
  if (!(W > 0.0)) return false;
  double pb[3], xb[3], S[3][3];
  for (int i = 0; i < 3; ++i) { pb[i] = s[1 + i] / W; xb[i] = s[4 + i] / W; }
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) S[i][k] = s[7 + i * 3 + k] - s[1 + i] * xb[k];
  double A[4][4], V[4][4];
  A[0][0] = (S[0][0] + S[1][1]) + S[2][2];
  A[1][1] = (S[0][0] - S[1][1]) - S[2][2];
  A[2][2] = (S[1][1] - S[0][0]) - S[2][2];
  A[3][3] = (S[2][2] - S[0][0]) - S[1][1];
  A[0][1] = A[1][0] = S[1][2] - S[2][1];
  A[0][2] = A[2][0] = S[2][0] - S[0][2];
  A[0][3] = A[3][0] = S[0][1] - S[1][0];
  A[1][2] = A[2][1] = S[0][1] + S[1][0];
  A[1][3] = A[3][1] = S[2][0] + S[0][2];
  A[2][3] = A[3][2] = S[1][2] + S[2][1];
  jacobi4(A, V);
  const double ev[4] = {A[0][0], A[1][1], A[2][2], A[3][3]};
  int best = 0;
  for (int k = 1; k < 4; ++k)
    if (ev[k] > ev[best]) best = k;
  double second = -INFINITY, scale = 0.0;
  for (int k = 0; k < 4; ++k) {
    if (k != best) second = fmax(second, ev[k]);
    scale = fmax(scale, fabs(ev[k]));
  }
  if (!(ev[best] - second > MIN_GAP * scale)) return false;     // (NaN sums end here too)
  double q[4];
  for (int i = 0; i < 4; ++i) {
    q[i] = V[i][0];
    for (int k = 1; k < 4; ++k)
      if (k == best) q[i] = V[i][k];
  }
  const double nq = sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));
  for (int i = 0; i < 4; ++i) q[i] /= nq;
  const double q0 = q[0], qx = q[1], qy = q[2], qz = q[3];
  R[0] = (q0 * q0 + qx * qx) - (qy * qy + qz * qz);
  R[1] = 2.0 * (qx * qy - q0 * qz);
  R[2] = 2.0 * (qx * qz + q0 * qy);
  R[3] = 2.0 * (qx * qy + q0 * qz);
  R[4] = (q0 * q0 + qy * qy) - (qx * qx + qz * qz);
  R[5] = 2.0 * (qy * qz - q0 * qx);
  R[6] = 2.0 * (qx * qz - q0 * qy);
  R[7] = 2.0 * (qy * qz + q0 * qx);
  R[8] = (q0 * q0 + qz * qz) - (qx * qx + qy * qy);
  for (int i = 0; i < 3; ++i) t[i] = xb[i] - ((R[i * 3 + 0] * pb[0] + R[i * 3 + 1] * pb[1]) + R[i * 3 + 2] * pb[2]);
  return true;
}

// acc[0..15] += the sixteen sums of one pair with weight w
__device__ __forceinline__ void add_pair(double w, const double* P, const double* X, double* acc) {
  acc[0] += w;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    acc[1 + i] += w * P[i];
    acc[4 + i] += w * X[i];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[7 + i * 3 + k] += (w * P[i]) * X[k];
}

__device__ __forceinline__ double area2(const double (*P)[3]) {
  double e1[3], e2[3];
  for (int i = 0; i < 3; ++i) { e1[i] = P[1][i] - P[0][i]; e2[i] = P[2][i] - P[0][i]; }
  const double c0 = e1[1] * e2[2] - e1[2] * e2[1], c1 = e1[2] * e2[0] - e1[0] * e2[2], c2 = e1[0] * e2[1] - e1[1] * e2[0];
  return sqrt((c0 * c0 + c1 * c1) + c2 * c2);
}

// |R p + t - x|^2, fp64
__device__ __forceinline__ double dist2(const double* R, const double* t, const double* P, const double* X) {
  double d[3];
  for (int i = 0; i < 3; ++i) d[i] = (((R[i * 3 + 0] * P[0] + R[i * 3 + 1] * P[1]) + R[i * 3 + 2] * P[2]) + t[i]) - X[i];
  return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
}

// grid (ceil(H / 256), B); dynamic LDS: the uint16 candidate list
__global__ __launch_bounds__(NT) void kabsch_hyp_kernel(KabschArgs a, int* __restrict__ samples, float* __restrict__ hp,
                                                        int* __restrict__ counts) {
  extern __shared__ unsigned short list[];
  __shared__ int wave_tot[NT / 64];
  const int b = blockIdx.y;
  const int k = blockIdx.x * NT + threadIdx.x;
  const float* r = a.rec + (size_t)b * a.h * a.w * a.ld;
  const float* cp = a.cam + (size_t)b * a.h * a.w * a.ldp;
  const int n = build_candidates(a, r, cp, list, wave_tot);
  if (k >= a.H) return;
  int s[3] = {-1, -1, -1};
  int got = 0;
  if (n >= a.min_points) {
    const uint32_t frame = (uint32_t)(a.t0 + b);
    const uint32_t key = a.seed ^ (frame * 0x9E3779B1u) ^ ((uint32_t)k * 0x85EBCA77u);
    for (int draw = 0; draw < MAX_DRAWS && got < 3; ++draw) {
      const uint32_t hsh = lowbias32(key ^ ((uint32_t)draw * 0xC2B2AE3Du));
      const int idx = (int)(((uint64_t)hsh * (uint64_t)n) >> 32);
      bool dup = false;
      for (int i = 0; i < got; ++i) dup |= s[i] == idx;
      if (!dup) s[got++] = idx;
    }
  }
  const bool sampled = got == 3;
  const size_t hk = (size_t)b * a.H + k;
  if (samples)
    for (int i = 0; i < 3; ++i) samples[hk * 3 + i] = sampled ? s[i] : -1;
  double R[9], t[3];
  bool ok = false;
  if (sampled) {
    double P[3][3], X[3][3], acc[16];
    for (int i = 0; i < 16; ++i) acc[i] = 0.0;
    for (int i = 0; i < 3; ++i) {
      load_pair(a, r, cp, list[s[i]], P[i], X[i]);
      add_pair(1.0, P[i], X[i], acc);
    }
    ok = !(area2(P) < MIN_AREA2) && !(area2(X) < MIN_AREA2) && kabsch_from_sums(acc, R, t);
  }
  float* o = hp + hk * 12;
  for (int rr = 0; rr < 3; ++rr) {
    for (int c = 0; c < 3; ++c) o[rr * 4 + c] = ok ? (float)R[rr * 3 + c] : __builtin_nanf("");
    o[rr * 4 + 3] = ok ? (float)t[rr] : __builtin_nanf("");
  }
  counts[hk] = ok ? 0 : -1;
}

// grid (ceil(h*w / TILE), ceil(H / 256), B).  d = R p + t - x with the products fused; inlier iff |d|^2 < inlier_m^2, fp32.
__global__ __launch_bounds__(NT) void kabsch_score_kernel(KabschArgs a, const float* __restrict__ hp, int* __restrict__ counts) {
  __shared__ f32x4 sp[TILE];      // Xc, Yc, Zc, x
  __shared__ f32x2 sq[TILE];      // y, z
  __shared__ int wave_tot[NT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int b = blockIdx.z;
  const int hw = a.h * a.w;
  const float* r = a.rec + (size_t)b * hw * a.ld;
  const float* cp = a.cam + (size_t)b * hw * a.ldp;
  const int c = blockIdx.x * TILE + tid;
  f32x4 P = {0.f, 0.f, 0.f, 0.f};
  f32x2 Q = {0.f, 0.f};
  bool keep = false;
  if (tid < TILE && c < hw) {
    const float* x = r + (size_t)c * a.ld;
    const float* p = cp + (size_t)c * a.ldp;
    keep = is_candidate(x, p, a.minc);
    P = f32x4{p[0], p[1], p[2], x[0]};
    Q = f32x2{x[1], x[2]};
  }
  const unsigned long long m = __ballot(keep);
  if (lane == 0) wave_tot[wv] = __popcll(m);
  __syncthreads();
  int off = 0;
  for (int k = 0; k < wv; ++k) off += wave_tot[k];
  if (keep) {
    const int j = off + __popcll(m & ((1ull << lane) - 1ull));     // j < TILE: only the first TILE threads keep
    sp[j] = P;
    sq[j] = Q;
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
  const float thr2 = a.thr * a.thr;
  int cnt = 0;
  for (int j = 0; j < nt; ++j) {
    const f32x4 p = sp[j];
    const f32x2 yz = sq[j];
    const float dx = fmaf(r00, p.x, fmaf(r01, p.y, fmaf(r02, p.z, tx))) - p.w;
    const float dy = fmaf(r10, p.x, fmaf(r11, p.y, fmaf(r12, p.z, ty))) - yz.x;
    const float dz = fmaf(r20, p.x, fmaf(r21, p.y, fmaf(r22, p.z, tz))) - yz.y;
    cnt += fmaf(dx, dx, fmaf(dy, dy, dz * dz)) < thr2 ? 1 : 0;
  }
  if (cnt) atomicAdd(&counts[hk], cnt);
}

// ---- selection + closed-form refinement ---------------------------------------------------------------------------------

constexpr int NV = 23;   // the last pass: 21 (upper triangle of sum w J^T J) + cost + inliers; the rounds use 17 of them

// Sum over the block in a fixed order: xor butterfly in each wave, then the four wave partials in wave order.  `red` holds
// [4][N] doubles, `out` receives N sums; every thread returns after `out` is valid.
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

// Most inliers among counts[0..H), ties to the lowest index; -1 when every count is negative.  Every thread of the block
// takes part and returns the same (index, count).
__device__ int select_best(const int* __restrict__ counts, int H, int* best_c, int* best_k, int* count_out) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int bc = -1, bk = -1;
  for (int k = tid; k < H; k += NT) {
    const int c = counts[k];
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
  *count_out = best_c[0];
  return best_k[0];
}

// grid (B): the probe of the selection rule alone
__global__ __launch_bounds__(NT) void kabsch_select_kernel(const int* __restrict__ counts, int H, int* __restrict__ best) {
  __shared__ int best_c[NT / 64], best_k[NT / 64];
  int count;
  const int k = select_best(counts + (size_t)blockIdx.x * H, H, best_c, best_k, &count);
  if (threadIdx.x == 0) best[blockIdx.x] = count < 0 ? -1 : k;
}

// Sigma = H^-1 from the Cholesky factor of the 6x6 H whose upper triangle is h[0..20] (row by row): L^-1 by forward
// substitution, Sigma = L^-T L^-1 with the upper triangle computed and mirrored, so Sigma is symmetric to the last bit.
// Returns false (Sigma untouched) if H is not positive definite.  (kfn_pnp.hip's routine, statement for statement.)
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

// grid (B); dynamic LDS: the uint16 candidate list.  cov and quality may be null.
__global__ __launch_bounds__(NT) void kabsch_refine_kernel(KabschArgs a, const float* __restrict__ hp,
                                                           const int* __restrict__ counts, float* __restrict__ poses,
                                                           float* __restrict__ cov, float* __restrict__ quality,
                                                           int* __restrict__ info) {
  extern __shared__ unsigned short list[];
  __shared__ int wave_tot[NT / 64];
  __shared__ int best_c[NT / 64], best_k[NT / 64];
  __shared__ double red[4 * NV];
  __shared__ double sums[NV];
  __shared__ double pose[12];   // R row-major, t: x = R p + t
  __shared__ int stop;
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const float* r = a.rec + (size_t)b * a.h * a.w * a.ld;
  const float* cp = a.cam + (size_t)b * a.h * a.w * a.ldp;
  const int n = build_candidates(a, r, cp, list, wave_tot);
  const double thr2 = (double)a.thr * (double)a.thr;

  int best_count;
  const int best = select_best(counts + (size_t)b * a.H, a.H, best_c, best_k, &best_count);
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

  // A lane's candidates are j = tid + 256 i, i < 128: its share of the inlier set is two 64-bit masks.
  unsigned long long prev0 = 0ull, prev1 = 0ull;
  for (int it = 0; it < a.iters; ++it) {
    double acc[17];
#pragma unroll
    for (int i = 0; i < 17; ++i) acc[i] = 0.0;
    unsigned long long cur0 = 0ull, cur1 = 0ull;
    int i = 0;
    for (int j = tid; j < n; j += NT, ++i) {
      double P[3], X[3];
      load_pair(a, r, cp, list[j], P, X);
      if (!(dist2(pose, pose + 9, P, X) < thr2)) continue;
      if (i < 64) cur0 |= 1ull << i; else cur1 |= 1ull << (i - 64);
      const double w = a.weighted ? 1.0 / (sigma2_of(a, r, list[j]) + a.ps2) : 1.0;
      add_pair(w, P, X, acc);
      acc[16] += 1.0;
    }
    // the same inlier set as the round before gives the same sums and the same pose: stop
    const int changed = __syncthreads_or((cur0 != prev0 || cur1 != prev1) ? 1 : 0);
    if (it > 0 && !changed) break;
    prev0 = cur0;
    prev1 = cur1;
    block_sum(acc, red, sums);
    if (tid == 0) {
      double R[9], t[3];
      if (sums[16] >= 3.0 && kabsch_from_sums(sums, R, t)) {
        for (int k = 0; k < 9; ++k) pose[k] = R[k];
        for (int k = 0; k < 3; ++k) pose[9 + k] = t[k];
      } else {
        stop = 1;      // fewer than 3 inliers or a degenerate set: the previous pose stays
      }
    }
    __syncthreads();
    if (stop) break;
  }

  // the final inliers and, with w = 1 / (sigma^2 + point_sigma^2) in both modes, their normal equations in the coordinates
  // (omega, tau) of the left perturbation of the world-to-camera pose: q = R^T (x - t), J = [-[q]x | I]
  double acc[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) acc[i] = 0.0;
  for (int j = tid; j < n; j += NT) {
    double P[3], X[3];
    load_pair(a, r, cp, list[j], P, X);
    const double d2 = dist2(pose, pose + 9, P, X);
    if (!(d2 < thr2)) continue;
    const double w = 1.0 / (sigma2_of(a, r, list[j]) + a.ps2);
    double e[3], q[3];
    for (int k = 0; k < 3; ++k) e[k] = X[k] - pose[9 + k];
    for (int k = 0; k < 3; ++k) q[k] = (pose[0 * 3 + k] * e[0] + pose[1 * 3 + k] * e[1]) + pose[2 * 3 + k] * e[2];
    const double J0[6] = {0.0, q[2], -q[1], 1.0, 0.0, 0.0};
    const double J1[6] = {-q[2], 0.0, q[0], 0.0, 1.0, 0.0};
    const double J2[6] = {q[1], -q[0], 0.0, 0.0, 0.0, 1.0};
    int m = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int k = i; k < 6; ++k) acc[m++] += w * ((J0[i] * J0[k] + J1[i] * J1[k]) + J2[i] * J2[k]);
    acc[21] += w * d2;
    acc[22] += 1.0;
  }
  block_sum(acc, red, sums);
  const int inliers = (int)sums[22];
  if (tid == 0) {
    double Sg[6][6];
    const bool pd = inliers >= 3 && inverse_spd6(sums, Sg);
    if (cov)
      for (int i = 0; i < 36; ++i) cov[(size_t)b * 36 + i] = pd ? (float)Sg[i / 6][i % 6] : __builtin_nanf("");
    if (quality) {
      quality[(size_t)b * 2 + 0] = (float)sums[21];
      quality[(size_t)b * 2 + 1] = (float)(3 * inliers - 6);
    }
  }
  if (tid < 16) {
    const int rr = tid / 4, c = tid % 4;
    double val;
    if (rr == 3) val = (c == 3) ? 1.0 : 0.0;
    else val = c < 3 ? pose[rr * 3 + c] : pose[9 + rr];
    poses[(size_t)b * 16 + tid] = (float)val;
  }
  if (tid == 0) {
    info[b * 4 + 0] = KFN_PNP_OK; info[b * 4 + 1] = n; info[b * 4 + 2] = inliers; info[b * 4 + 3] = best;
  }
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Copy of the caller's descriptor and the argument checks shared by the entry points.
int kabsch_desc_in(const kfn_kabsch_desc* in, kfn_kabsch_desc* d, const char* who) {
  if (in == nullptr) return kfn::fail(KFN_ERR_ARG, "%s: null descriptor", who);
  const int32_t sz = in->struct_size;
  if (sz < (int32_t)sizeof(kfn_kabsch_desc) || (sz & 3) != 0)
    return kfn::fail(KFN_ERR_ARG, "%s: kfn_kabsch_desc.struct_size = %d (this library: %d bytes) -- use KFN_KABSCH_DESC_INIT",
                     who, (int)sz, (int)sizeof(kfn_kabsch_desc));
  std::memcpy(d, in, sizeof(*d));   // (a larger struct from a newer host: its tail is not read)
  KFN_REQUIRE(d->B > 0 && d->h > 0 && d->w > 0, "%s: bad shape B=%d h=%d w=%d", who, d->B, d->h, d->w);
  KFN_REQUIRE((long)d->h * d->w <= MAX_CELLS, "%s: h*w = %ld cells, at most %d", who, (long)d->h * d->w, MAX_CELLS);
  KFN_REQUIRE(d->ld >= 4, "%s: ld = %d < 4", who, d->ld);
  KFN_REQUIRE(d->ldp >= 4, "%s: ldp = %d < 4", who, d->ldp);
  KFN_REQUIRE(d->t0 >= 0, "%s: t0 = %d < 0", who, d->t0);
  KFN_REQUIRE(d->hypotheses >= 1 && d->hypotheses <= KFN_PNP_MAX_HYPOTHESES, "%s: hypotheses = %d (1..%d)", who,
              d->hypotheses, KFN_PNP_MAX_HYPOTHESES);
  KFN_REQUIRE(d->refine_iters >= 0 && d->refine_iters <= 100, "%s: refine_iters = %d (0..100)", who, d->refine_iters);
  KFN_REQUIRE(d->min_points >= 3, "%s: min_points = %d < 3", who, d->min_points);
  KFN_REQUIRE(d->min_confidence >= 0.f, "%s: min_confidence = %g, must be >= 0 (sigma = 1 / confidence must be positive)", who,
              (double)d->min_confidence);
  KFN_REQUIRE(d->inlier_m > 0.f && std::isfinite(d->inlier_m), "%s: inlier_m = %g, must be > 0", who, (double)d->inlier_m);
  KFN_REQUIRE(d->weighted == 0 || d->weighted == 1, "%s: weighted = %d (0 or 1)", who, d->weighted);
  KFN_REQUIRE(d->point_sigma > 0.f && std::isfinite(d->point_sigma), "%s: point_sigma = %g, must be > 0", who,
              (double)d->point_sigma);
  return KFN_OK;
}

KabschArgs kabsch_args(const kfn_kabsch_desc* d, const float* records, const float* cam_points) {
  KabschArgs a;
  a.rec = records;
  a.cam = cam_points;
  a.B = d->B; a.h = d->h; a.w = d->w; a.ld = d->ld; a.ldp = d->ldp; a.t0 = d->t0;
  a.seed = d->seed;
  a.H = d->hypotheses; a.iters = d->refine_iters; a.min_points = d->min_points;
  a.minc = d->min_confidence; a.thr = d->inlier_m;
  a.weighted = d->weighted;
  a.ps2 = (double)d->point_sigma * (double)d->point_sigma;
  return a;
}

int launch_hyp_and_score(const KabschArgs& a, int* samples, float* hp, int* counts, hipStream_t st) {
  static std::atomic<uint64_t> hyp_lds_done{0};
  const int rc = kfn::set_max_dynamic_lds((const void*)kabsch_hyp_kernel, 2 * MAX_CELLS, hyp_lds_done);
  if (rc != KFN_OK) return rc;
  const unsigned hb = (unsigned)kfn::ceil_div(a.H, NT);
  hipLaunchKernelGGL(kabsch_hyp_kernel, dim3(hb, (unsigned)a.B), dim3(NT), 2 * a.h * a.w, st, a, samples, hp, counts);
  KFN_LAUNCH_CHECK("kabsch_hyp_kernel");
  hipLaunchKernelGGL(kabsch_score_kernel, dim3((unsigned)kfn::ceil_div(a.h * a.w, TILE), hb, (unsigned)a.B), dim3(NT), 0, st, a,
                     (const float*)hp, counts);
  KFN_LAUNCH_CHECK("kabsch_score_kernel");
  return KFN_OK;
}

}  // namespace

extern "C" int kfn_kabsch_scratch_bytes(const kfn_kabsch_desc* desc, size_t* bytes) {
  kfn_kabsch_desc d;
  const int rc = kabsch_desc_in(desc, &d, "kfn_kabsch_scratch_bytes");
  if (rc != KFN_OK) return rc;
  KFN_REQUIRE(bytes, "kfn_kabsch_scratch_bytes: null bytes");
  const size_t bh = (size_t)d.B * d.hypotheses;
  *bytes = align256(bh * 12 * sizeof(float)) + align256(bh * sizeof(int32_t));
  return KFN_OK;
}

extern "C" int kfn_kabsch_ransac(const kfn_kabsch_desc* desc, const float* records, const float* cam_points, float* poses,
                                 float* cov, float* quality, int32_t* info, void* scratch, void* stream) {
  kfn_kabsch_desc d;
  int rc = kabsch_desc_in(desc, &d, "kfn_kabsch_ransac");
  if (rc != KFN_OK) return rc;
  KFN_REQUIRE(records && cam_points && poses && info && scratch, "kfn_kabsch_ransac: null argument");
  KFN_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 15) == 0, "kfn_kabsch_ransac: scratch not 16-byte aligned");
  const KabschArgs a = kabsch_args(&d, records, cam_points);
  const size_t bh = (size_t)d.B * d.hypotheses;
  float* hp = static_cast<float*>(scratch);
  int* counts = reinterpret_cast<int*>(static_cast<char*>(scratch) + align256(bh * 12 * sizeof(float)));
  const hipStream_t st = (hipStream_t)stream;
  static std::atomic<uint64_t> ref_lds_done{0};
  rc = kfn::set_max_dynamic_lds((const void*)kabsch_refine_kernel, 2 * MAX_CELLS, ref_lds_done);
  if (rc != KFN_OK) return rc;
  rc = launch_hyp_and_score(a, nullptr, hp, counts, st);
  if (rc != KFN_OK) return rc;
  hipLaunchKernelGGL(kabsch_refine_kernel, dim3((unsigned)d.B), dim3(NT), 2 * d.h * d.w, st, a, (const float*)hp,
                     (const int*)counts, poses, cov, quality, info);
  KFN_LAUNCH_CHECK("kabsch_refine_kernel");
  return KFN_OK;
}

extern "C" int kfn_kabsch_hypotheses(const kfn_kabsch_desc* desc, const float* records, const float* cam_points,
                                     int32_t* samples, float* hyp_poses, int32_t* counts, void* stream) {
  kfn_kabsch_desc d;
  const int rc = kabsch_desc_in(desc, &d, "kfn_kabsch_hypotheses");
  if (rc != KFN_OK) return rc;
  KFN_REQUIRE(records && cam_points && samples && hyp_poses && counts, "kfn_kabsch_hypotheses: null argument");
  return launch_hyp_and_score(kabsch_args(&d, records, cam_points), samples, hyp_poses, counts, (hipStream_t)stream);
}

extern "C" int kfn_kabsch_select(const int32_t* counts, int B, int hypotheses, int32_t* best, void* stream) {
  KFN_REQUIRE(B > 0, "kfn_kabsch_select: B = %d", B);
  KFN_REQUIRE(hypotheses >= 1 && hypotheses <= KFN_PNP_MAX_HYPOTHESES, "kfn_kabsch_select: hypotheses = %d (1..%d)", hypotheses,
              KFN_PNP_MAX_HYPOTHESES);
  KFN_REQUIRE(counts && best, "kfn_kabsch_select: null argument");
  hipLaunchKernelGGL(kabsch_select_kernel, dim3((unsigned)B), dim3(NT), 0, (hipStream_t)stream, (const int*)counts, hypotheses,
                     best);
  KFN_LAUNCH_CHECK("kabsch_select_kernel");
  return KFN_OK;
}
