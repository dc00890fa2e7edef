// kfn_pose_track.hip -- the pose tracker: kfn_pose_filter's random walk or a constant-velocity model, forwards over the
// per-frame camera poses of kfn_pnp_ransac_unc, an optional backward (Rauch-Tung-Striebel) pass over the frames of the
// call, and a state that is carried from call to call.
//
// One sequence per lane, fp64, serial over t, as kfn_pose_filter.hip.  The kernel is a template over n, the size of the
// error state: n = 6 (dtheta, drho) for the walk, n = 12 (dtheta, drho, domega, dv) for the velocity model, whose state
// also holds the body-frame twist xi = (omega, v) per frame.  DESIGN.md 5c "Pose tracker" fixes every step, and
// tests/pose_track_ref.py restates them in numpy; built with -ffp-contract=off.
//
// Where the matrices live:
//   n = 6    the forward pass is pose_filter_kernel's text: P and its five 6x6 work arrays are private, as there.
//   n = 12   P (12x12) is in LDS, element-major with the lane innermost (144 * 64 doubles per block); the gain, the
//            Joseph form and the prediction work on it in place in 6x6 blocks, so the private arrays are the six 6x6 ones
//            of the walk.
//   backward every frame's filtered and predicted (R, p, xi, P) go to `scratch`, element-major with the sequence
//            innermost, so that the 64 lanes of a block touch consecutive addresses; a second launch on the same stream
//            (pose_smooth_kernel, same lane = same sequence) factors P_p, builds the gain C and the smoothed estimate
//            in that memory (the smoothed estimate replaces the filtered one of its frame).
//
// Approximations: S = P + Sigma_z as in kfn_pose_filter.hip; F = [[I, I], [0, I]] takes the adjoint of exp(-xi) and the
// right Jacobian as the identity (first order in one frame's motion); the smoother applies a correction expressed in
// frame t+1's predicted body frame in frame t's (the same order).
#include <cmath>

#include "kfn_common.h"

namespace {

constexpr int LANES = 64;
constexpr int P12_LDS_BYTES = 144 * LANES * (int)sizeof(double);

struct TrackArgs {
  const float* poses;
  const float* cov;
  double* state;          // [2 + slot doubles][S], or null
  float* out_poses;
  float* out_cov;
  int* flags;
  float* nis;
  float* smooth_poses;    // null unless smooth
  float* smooth_cov;
  double* scratch;        // [T][2][slot doubles][S] history, then C and D [2][n * n][S]; null unless smooth
  int S, T, max_rejects, smooth;
  double qr, qt, gate;    // rot_sigma^2, trans_sigma^2, the NIS gate
  double rr, rt;          // rot_rate_sigma^2, trans_rate_sigma^2 (n = 12)
};

// A slot is one estimate in memory: R (9), p (3), xi (n - 6), P (n * n).
constexpr int slot_p(int n) { return 12 + (n - 6); }
constexpr int slot_doubles(int n) { return slot_p(n) + n * n; }

// In-place Cholesky of the symmetric A: the lower triangle becomes L.  false if A is not positive definite.
__device__ __noinline__ bool chol6(double (*A)[6]) {
  for (int j = 0; j < 6; ++j) {
    double s = A[j][j];
    for (int k = 0; k < j; ++k) s -= A[j][k] * A[j][k];
    if (!(s > 0.0)) return false;
    A[j][j] = sqrt(s);
    for (int i = j + 1; i < 6; ++i) {
      double t = A[i][j];
      for (int k = 0; k < j; ++k) t -= A[i][k] * A[j][k];
      A[i][j] = t / A[j][j];
    }
  }
  return true;
}

__device__ __noinline__ void forward6(double (*L)[6], const double* b, double* y) {
  for (int i = 0; i < 6; ++i) {
    double s = b[i];
    for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
    y[i] = s / L[i][i];
  }
}

__device__ __noinline__ void backward6(double (*L)[6], const double* y, double* x) {
  for (int i = 5; i >= 0; --i) {
    double s = y[i];
    for (int k = i + 1; k < 6; ++k) s -= L[k][i] * x[k];
    x[i] = s / L[i][i];
  }
}

// Rodrigues' formula, as pnp_refine_kernel's
__device__ __noinline__ void exp_so3(const double* w, double* E) {
  const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
  const double s1 = th < 1e-12 ? 1.0 : sin(th) / th;
  const double s2 = th < 1e-12 ? 0.0 : (1.0 - cos(th)) / (th * th);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      const double kk = K[r * 3 + 0] * K[0 * 3 + c] + K[r * 3 + 1] * K[1 * 3 + c] + K[r * 3 + 2] * K[2 * 3 + c];
      E[r * 3 + c] = ((r == c) ? 1.0 : 0.0) + s1 * K[r * 3 + c] + s2 * kk;
    }
}

// w with exp(w) ~ M: the angle from atan2(|skew part|, (trace - 1) / 2), the axis from the skew part
__device__ __noinline__ void log_so3(const double* M, double* w) {
  const double c = ((M[0] + M[4] + M[8]) - 1.0) / 2.0;
  const double k[3] = {(M[7] - M[5]) / 2.0, (M[2] - M[6]) / 2.0, (M[3] - M[1]) / 2.0};
  const double s = sqrt(k[0] * k[0] + k[1] * k[1] + k[2] * k[2]);
  const double f = s < 1e-12 ? 1.0 : atan2(s, c) / s;
  for (int i = 0; i < 3; ++i) w[i] = f * k[i];
}

// ---- n = 12: P in LDS, element (i, j) of this lane at Pl[(i * 12 + j) * LANES] -----------------------------------------
#define P12(i, j) Pl[((i) * 12 + (j)) * LANES]

// P <- F P F^T + Q with F = [[I, I], [0, I]], block by block: with P = [[A, B], [B^T, D]] the pose block becomes
// ((A + B) + B^T) + D (upper triangle, mirrored), the cross block B + D; then Q = [[q/3, q/2], [q/2, q]] per axis.
__device__ __noinline__ void predict12(double* Pl, double qr, double qt) {
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) {
      const double v = ((P12(i, j) + P12(i, 6 + j)) + P12(j, 6 + i)) + P12(6 + i, 6 + j);
      P12(i, j) = v;
      P12(j, i) = v;
    }
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) {
      const double v = P12(i, 6 + j) + P12(6 + i, 6 + j);
      P12(i, 6 + j) = v;
      P12(6 + j, i) = v;
    }
  for (int i = 0; i < 6; ++i) {
    const double q = (i < 3) ? qr : qt;
    P12(i, i) += q / 3.0;
    const double v = P12(i, 6 + i) + q / 2.0;
    P12(i, 6 + i) = v;
    P12(6 + i, i) = v;
    P12(6 + i, 6 + i) += q;
  }
}

// Joseph form (I - K H) P (I - K H)^T + K Sigma_z K^T in place, with I - K H = [[A, 0], [-K2, I]], A = I - K1, and
// KS1 = K1 Sigma_z, KS2 = K2 Sigma_z.  First (I - K H) P column by column, then the upper triangle of the products row by
// row (row i reads only its own row), then the mirror: P stays symmetric to the last bit.
__device__ __noinline__ void joseph12(double* Pl, double (*A)[6], double (*K1)[6], double (*K2)[6], double (*KS1)[6],
                                      double (*KS2)[6]) {
  for (int j = 0; j < 12; ++j) {
    double c[6];
    for (int k = 0; k < 6; ++k) c[k] = P12(k, j);
    for (int i = 0; i < 6; ++i) {
      double s1 = 0.0, s2 = 0.0;
      for (int k = 0; k < 6; ++k) { s1 += A[i][k] * c[k]; s2 += K2[i][k] * c[k]; }
      P12(i, j) = s1;
      P12(6 + i, j) = P12(6 + i, j) - s2;
    }
  }
  for (int i = 0; i < 12; ++i) {
    double r[6];
    for (int k = 0; k < 6; ++k) r[k] = P12(i, k);
    const double* ks = (i < 6) ? KS1[i] : KS2[i - 6];
    for (int j = i; j < 12; ++j) {
      double s1 = 0.0, s2 = 0.0;
      if (j < 6) {
        for (int k = 0; k < 6; ++k) { s1 += r[k] * A[j][k]; s2 += ks[k] * K1[j][k]; }
      } else {
        for (int k = 0; k < 6; ++k) { s1 += r[k] * K2[j - 6][k]; s2 += ks[k] * K2[j - 6][k]; }
        s1 = P12(i, j) - s1;
      }
      P12(i, j) = s1 + s2;
    }
  }
  for (int i = 0; i < 12; ++i)
    for (int j = i + 1; j < 12; ++j) P12(j, i) = P12(i, j);
}

// ---- the backward pass: n x n matrices in global memory, element (i, j) at A[(i * n + j) * ld] ---------------------------

__device__ __noinline__ bool chol_mem(double* A, int n, size_t ld) {
  for (int j = 0; j < n; ++j) {
    double s = A[(size_t)(j * n + j) * ld];
    for (int k = 0; k < j; ++k) s -= A[(size_t)(j * n + k) * ld] * A[(size_t)(j * n + k) * ld];
    if (!(s > 0.0)) return false;
    const double djj = sqrt(s);
    A[(size_t)(j * n + j) * ld] = djj;
    for (int i = j + 1; i < n; ++i) {
      double t = A[(size_t)(i * n + j) * ld];
      for (int k = 0; k < j; ++k) t -= A[(size_t)(i * n + k) * ld] * A[(size_t)(j * n + k) * ld];
      A[(size_t)(i * n + j) * ld] = t / djj;
    }
  }
  return true;
}

// x <- (L L^T)^-1 x
__device__ __noinline__ void solve_mem(const double* L, int n, size_t ld, double* x) {
  for (int i = 0; i < n; ++i) {
    double s = x[i];
    for (int k = 0; k < i; ++k) s -= L[(size_t)(i * n + k) * ld] * x[k];
    x[i] = s / L[(size_t)(i * n + i) * ld];
  }
  for (int i = n - 1; i >= 0; --i) {
    double s = x[i];
    for (int k = i + 1; k < n; ++k) s -= L[(size_t)(k * n + i) * ld] * x[k];
    x[i] = s / L[(size_t)(i * n + i) * ld];
  }
}

// Frame t from frame t+1.  F0: the filtered estimate of t, replaced by the smoothed one; S1: the smoothed estimate of
// t+1; P1: the predicted estimate of t+1, whose P is replaced by its Cholesky factor; Cw, Dw: n x n work matrices.
// Leaves F0 as it is if P_p is not positive definite.
template <int N>
__device__ __noinline__ void smooth_step(double* F0, const double* S1, double* P1, double* Cw, double* Dw, size_t ld) {
  constexpr int OFF_P = slot_p(N);
  for (int e = 0; e < N * N; ++e) Dw[(size_t)e * ld] = S1[(size_t)(OFF_P + e) * ld] - P1[(size_t)(OFF_P + e) * ld];
  double* L = P1 + (size_t)OFF_P * ld;
  if (!chol_mem(L, N, ld)) return;
  // e = (log(R_p^T R_s), R_p^T (p_s - p_p), xi_s - xi_p) of frame t+1
  double Rp[9], Rs[9], M[9], e[N], d[N];
  for (int i = 0; i < 9; ++i) { Rp[i] = P1[(size_t)i * ld]; Rs[i] = S1[(size_t)i * ld]; }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) M[r * 3 + c] = Rp[0 * 3 + r] * Rs[0 * 3 + c] + Rp[1 * 3 + r] * Rs[1 * 3 + c] + Rp[2 * 3 + r] * Rs[2 * 3 + c];
  log_so3(M, e);
  const double dp[3] = {S1[(size_t)9 * ld] - P1[(size_t)9 * ld], S1[(size_t)10 * ld] - P1[(size_t)10 * ld],
                        S1[(size_t)11 * ld] - P1[(size_t)11 * ld]};
  for (int r = 0; r < 3; ++r) e[3 + r] = Rp[0 * 3 + r] * dp[0] + Rp[1 * 3 + r] * dp[1] + Rp[2 * 3 + r] * dp[2];
  for (int k = 6; k < N; ++k) e[k] = S1[(size_t)(6 + k) * ld] - P1[(size_t)(6 + k) * ld];
  // C = P_f F^T P_p^-1 row by row (P_p symmetric: row i of C solves P_p c = (P_f F^T)[i, :]); d = C e
  for (int i = 0; i < N; ++i) {
    double g[N];
    for (int j = 0; j < N; ++j) {
      g[j] = F0[(size_t)(OFF_P + i * N + j) * ld];
      if (N == 12 && j < 6) g[j] = g[j] + F0[(size_t)(OFF_P + i * N + j + 6) * ld];
    }
    solve_mem(L, N, ld, g);
    double sum = 0.0;
    for (int k = 0; k < N; ++k) {
      Cw[(size_t)(i * N + k) * ld] = g[k];
      sum += g[k] * e[k];
    }
    d[i] = sum;
  }
  // p_s = p_f + R_f d_rho, R_s = R_f exp(d_theta), xi_s = xi_f + d_xi
  double R[9], E[9];
  for (int i = 0; i < 9; ++i) R[i] = F0[(size_t)i * ld];
  for (int r = 0; r < 3; ++r) F0[(size_t)(9 + r) * ld] = F0[(size_t)(9 + r) * ld] + (R[r * 3 + 0] * d[3] + R[r * 3 + 1] * d[4] + R[r * 3 + 2] * d[5]);
  exp_so3(d, E);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) F0[(size_t)(r * 3 + c) * ld] = R[r * 3 + 0] * E[0 * 3 + c] + R[r * 3 + 1] * E[1 * 3 + c] + R[r * 3 + 2] * E[2 * 3 + c];
  for (int k = 6; k < N; ++k) F0[(size_t)(6 + k) * ld] = F0[(size_t)(6 + k) * ld] + d[k];
  // P_s = P_f + C (P_s,t+1 - P_p,t+1) C^T, upper triangle mirrored
  for (int i = 0; i < N; ++i) {
    double g[N];
    for (int l = 0; l < N; ++l) {
      double sum = 0.0;
      for (int k = 0; k < N; ++k) sum += Cw[(size_t)(i * N + k) * ld] * Dw[(size_t)(k * N + l) * ld];
      g[l] = sum;
    }
    for (int j = i; j < N; ++j) {
      double sum = 0.0;
      for (int l = 0; l < N; ++l) sum += g[l] * Cw[(size_t)(j * N + l) * ld];
      const double v = F0[(size_t)(OFF_P + i * N + j) * ld] + sum;
      F0[(size_t)(OFF_P + i * N + j) * ld] = v;
      F0[(size_t)(OFF_P + j * N + i) * ld] = v;
    }
  }
}

// grid (ceil(S / 64)), 64 threads: lane = sequence.  N = 12 needs P12_LDS_BYTES of dynamic LDS.
template <int N>
__global__ __launch_bounds__(LANES) void pose_track_kernel(TrackArgs a) {
  constexpr int OFF_P = slot_p(N), SLOT = slot_doubles(N);
  extern __shared__ __attribute__((aligned(16))) double lds_p[];
  const int s = blockIdx.x * LANES + threadIdx.x;
  if (s >= a.S) return;
  const double nan = __builtin_nan("");
  double* const Pl = lds_p + threadIdx.x;
  const size_t ld = (size_t)a.S;
  double* hist = a.scratch + s;     // this frame's two slots (smooth)
  const double qr = a.qr, qt = a.qt, gate = a.gate, rr = a.rr, rt = a.rt;
  bool have = false;
  int rejects = 0;
  double R[9], p[3], P[6][6], xi[6];
  for (int i = 0; i < 6; ++i) xi[i] = 0.0;
  if (a.state != nullptr) {
    const double* st = a.state + s;
    have = st[0] != 0.0;
    rejects = (int)st[ld];
    if (have) {
      st += 2 * ld;
      for (int i = 0; i < 9; ++i) R[i] = st[(size_t)i * ld];
      for (int i = 0; i < 3; ++i) p[i] = st[(size_t)(9 + i) * ld];
      if constexpr (N == 6) {
#pragma nounroll
        for (int i = 0; i < 36; ++i) P[i / 6][i % 6] = st[(size_t)(OFF_P + i) * ld];
      } else {
        for (int i = 0; i < 6; ++i) xi[i] = st[(size_t)(12 + i) * ld];
#pragma nounroll
        for (int i = 0; i < 144; ++i) Pl[i * LANES] = st[(size_t)(OFF_P + i) * ld];
      }
    }
  }
  // the current estimate -> a slot in memory
  auto store_slot = [&](double* dst) {
    for (int i = 0; i < 9; ++i) dst[(size_t)i * ld] = R[i];
    for (int i = 0; i < 3; ++i) dst[(size_t)(9 + i) * ld] = p[i];
    if constexpr (N == 6) {
#pragma nounroll
      for (int i = 0; i < 36; ++i) dst[(size_t)(OFF_P + i) * ld] = P[i / 6][i % 6];
    } else {
      for (int i = 0; i < 6; ++i) dst[(size_t)(12 + i) * ld] = xi[i];
#pragma nounroll
      for (int i = 0; i < 144; ++i) dst[(size_t)(OFF_P + i) * ld] = Pl[i * LANES];
    }
  };
  for (int t = 0; t < a.T; ++t) {
    const size_t f = (size_t)s * a.T + t;
    const float* z = a.poses + f * 16;
    const float* cz = a.cov + f * 36;
    // valid = every value finite, as pose_filter_kernel's chain of isfinite(), in integer arithmetic: an all-ones exponent
    // carries into bit 31.  (That chain is 48 nested branches, or 48 compare masks, which do not fit the scalar registers.)
    unsigned bad = 0u;
    for (int i = 0; i < 12; ++i) bad |= (__float_as_uint(z[i]) & 0x7f800000u) + 0x00800000u;
    for (int i = 0; i < 36; ++i) bad |= (__float_as_uint(cz[i]) & 0x7f800000u) + 0x00800000u;
    const bool valid = (bad >> 31) == 0u;
    double Rz[9], pz[3];
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) Rz[r * 3 + c] = (double)z[r * 4 + c];
      pz[r] = (double)z[r * 4 + 3];
    }
    int flag;
    double nisv = nan;
    bool init = false;
    if (!have) {
      flag = valid ? KFN_POSE_INIT : KFN_POSE_NONE;
      init = valid;
    } else {
      if constexpr (N == 6) {
        for (int i = 0; i < 6; ++i) P[i][i] += (i < 3) ? qr : qt;
      } else {
        // p <- p + R v, then R <- R exp(omega); xi is kept
        for (int r = 0; r < 3; ++r) p[r] += R[r * 3 + 0] * xi[3] + R[r * 3 + 1] * xi[4] + R[r * 3 + 2] * xi[5];
        double E[9], Rn[9];
        exp_so3(xi, E);
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 3; ++c) Rn[r * 3 + c] = R[r * 3 + 0] * E[0 * 3 + c] + R[r * 3 + 1] * E[1 * 3 + c] + R[r * 3 + 2] * E[2 * 3 + c];
        for (int i = 0; i < 9; ++i) R[i] = Rn[i];
        predict12(Pl, qr, qt);
      }
      if (a.smooth) store_slot(hist + (size_t)SLOT * ld);
      flag = KFN_POSE_MISSING;
      if (valid) {
        // innovation y = (log(R^T R_z), R^T (p_z - p)), S = P + Sigma_z = L L^T
        double M[9], y[6], L[6][6], u[6];
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 3; ++c) M[r * 3 + c] = R[0 * 3 + r] * Rz[0 * 3 + c] + R[1 * 3 + r] * Rz[1 * 3 + c] + R[2 * 3 + r] * Rz[2 * 3 + c];
        log_so3(M, y);
        const double dp[3] = {pz[0] - p[0], pz[1] - p[1], pz[2] - p[2]};
        for (int r = 0; r < 3; ++r) y[3 + r] = R[0 * 3 + r] * dp[0] + R[1 * 3 + r] * dp[1] + R[2 * 3 + r] * dp[2];
        if constexpr (N == 6) {
          for (int i = 0; i < 6; ++i)
            for (int j = 0; j < 6; ++j) L[i][j] = P[i][j] + (double)cz[i * 6 + j];
        } else {
          for (int i = 0; i < 6; ++i)
            for (int j = 0; j < 6; ++j) L[i][j] = P12(i, j) + (double)cz[i * 6 + j];
        }
        if (chol6(L)) {
          forward6(L, y, u);
          nisv = 0.0;
          for (int i = 0; i < 6; ++i) nisv += u[i] * u[i];
          if (nisv > gate) {
            ++rejects;
            flag = KFN_POSE_REJECTED;
            if (rejects >= a.max_rejects) { flag = KFN_POSE_INIT; init = true; }
          } else if constexpr (N == 6) {
            // K = P S^-1 row by row (S and P symmetric: row i of K solves S k = P[i,:]); delta = K y
            double K[6][6], d[6], A[6][6], AP[6][6], KS[6][6];
#pragma nounroll
            for (int i = 0; i < 6; ++i) {
              double w[6];
              forward6(L, P[i], w);
              backward6(L, w, K[i]);
            }
            for (int i = 0; i < 6; ++i) {
              double sum = 0.0;
              for (int k = 0; k < 6; ++k) sum += K[i][k] * y[k];
              d[i] = sum;
            }
            for (int r = 0; r < 3; ++r) p[r] += R[r * 3 + 0] * d[3] + R[r * 3 + 1] * d[4] + R[r * 3 + 2] * d[5];
            double E[9], Rn[9];
            exp_so3(d, E);
            for (int r = 0; r < 3; ++r)
              for (int c = 0; c < 3; ++c) Rn[r * 3 + c] = R[r * 3 + 0] * E[0 * 3 + c] + R[r * 3 + 1] * E[1 * 3 + c] + R[r * 3 + 2] * E[2 * 3 + c];
            for (int i = 0; i < 9; ++i) R[i] = Rn[i];
            // Joseph form, upper triangle mirrored: P stays symmetric to the last bit
            for (int i = 0; i < 6; ++i)
              for (int j = 0; j < 6; ++j) A[i][j] = ((i == j) ? 1.0 : 0.0) - K[i][j];
#pragma nounroll
            for (int i = 0; i < 6; ++i)
              for (int j = 0; j < 6; ++j) {
                double s1 = 0.0, s2 = 0.0;
                for (int k = 0; k < 6; ++k) { s1 += A[i][k] * P[k][j]; s2 += K[i][k] * (double)cz[k * 6 + j]; }
                AP[i][j] = s1;
                KS[i][j] = s2;
              }
#pragma nounroll
            for (int i = 0; i < 6; ++i)
              for (int j = i; j < 6; ++j) {
                double s1 = 0.0, s2 = 0.0;
                for (int k = 0; k < 6; ++k) { s1 += AP[i][k] * A[j][k]; s2 += KS[i][k] * K[j][k]; }
                P[i][j] = s1 + s2;
                P[j][i] = s1 + s2;
              }
            flag = KFN_POSE_UPDATED;
            rejects = 0;
          } else {
            // K = P[:, :6] S^-1 as K1 (pose rows) and K2 (rate rows), row by row as above; delta = K y
            double K1[6][6], K2[6][6], d[6], A[6][6], KS1[6][6], KS2[6][6];
#pragma nounroll
            for (int i = 0; i < 6; ++i) {
              double b[6], w[6];
              for (int k = 0; k < 6; ++k) b[k] = P12(i, k);
              forward6(L, b, w);
              backward6(L, w, K1[i]);
              for (int k = 0; k < 6; ++k) b[k] = P12(6 + i, k);
              forward6(L, b, w);
              backward6(L, w, K2[i]);
            }
            for (int i = 0; i < 6; ++i) {
              double sum = 0.0, sum2 = 0.0;
              for (int k = 0; k < 6; ++k) { sum += K1[i][k] * y[k]; sum2 += K2[i][k] * y[k]; }
              d[i] = sum;
              xi[i] += sum2;
            }
            for (int r = 0; r < 3; ++r) p[r] += R[r * 3 + 0] * d[3] + R[r * 3 + 1] * d[4] + R[r * 3 + 2] * d[5];
            double E[9], Rn[9];
            exp_so3(d, E);
            for (int r = 0; r < 3; ++r)
              for (int c = 0; c < 3; ++c) Rn[r * 3 + c] = R[r * 3 + 0] * E[0 * 3 + c] + R[r * 3 + 1] * E[1 * 3 + c] + R[r * 3 + 2] * E[2 * 3 + c];
            for (int i = 0; i < 9; ++i) R[i] = Rn[i];
            for (int i = 0; i < 6; ++i)
              for (int j = 0; j < 6; ++j) {
                double s1 = 0.0, s2 = 0.0;
                for (int k = 0; k < 6; ++k) { s1 += K1[i][k] * (double)cz[k * 6 + j]; s2 += K2[i][k] * (double)cz[k * 6 + j]; }
                A[i][j] = ((i == j) ? 1.0 : 0.0) - K1[i][j];
                KS1[i][j] = s1;
                KS2[i][j] = s2;
              }
            joseph12(Pl, A, K1, K2, KS1, KS2);
            flag = KFN_POSE_UPDATED;
            rejects = 0;
          }
        }
      }
    }
    if (init) {
      for (int i = 0; i < 9; ++i) R[i] = Rz[i];
      for (int i = 0; i < 3; ++i) p[i] = pz[i];
      if constexpr (N == 6) {
        for (int i = 0; i < 6; ++i)
          for (int j = 0; j < 6; ++j) P[i][j] = (double)cz[i * 6 + j];
      } else {
        // xi = 0; the rate block is diag(rot_rate_sigma^2 I, trans_rate_sigma^2 I), the cross blocks are 0
        for (int i = 0; i < 6; ++i) xi[i] = 0.0;
        for (int i = 0; i < 12; ++i)
          for (int j = 0; j < 12; ++j)
            P12(i, j) = (i < 6 && j < 6) ? (double)cz[i * 6 + j] : ((i == j) ? ((i < 9) ? rr : rt) : 0.0);
      }
      have = true;
      rejects = 0;
    }
    if (a.smooth) {
      if (have) store_slot(hist);
      hist += (size_t)(2 * SLOT) * ld;
    }
    float* op = a.out_poses + f * 16;
    float* oc = a.out_cov + f * 36;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) op[r * 4 + c] = have ? (float)R[r * 3 + c] : __builtin_nanf("");
      op[r * 4 + 3] = have ? (float)p[r] : __builtin_nanf("");
    }
    for (int c = 0; c < 4; ++c) op[12 + c] = have ? ((c == 3) ? 1.f : 0.f) : __builtin_nanf("");
    if constexpr (N == 6) {
      for (int i = 0; i < 36; ++i) oc[i] = have ? (float)P[i / 6][i % 6] : __builtin_nanf("");
    } else {
      for (int i = 0; i < 36; ++i) oc[i] = have ? (float)P12(i / 6, i % 6) : __builtin_nanf("");
    }
    a.flags[f] = flag;
    a.nis[f] = (float)nisv;
  }
  if (a.state != nullptr) {
    double* st = a.state + s;
    st[0] = have ? 1.0 : 0.0;
    st[ld] = (double)rejects;
    if (have) store_slot(st + 2 * ld);
  }
}

// The backward pass over the history that pose_track_kernel<N> left in `scratch`, same grid: the last frame's smoothed
// estimate is its filtered one; no information crosses a (re-)initialisation.
template <int N>
__global__ __launch_bounds__(LANES) void pose_smooth_kernel(TrackArgs a) {
  constexpr int OFF_P = slot_p(N), SLOT = slot_doubles(N);
  const int s = blockIdx.x * LANES + threadIdx.x;
  if (s >= a.S) return;
  const size_t ld = (size_t)a.S;
  double* const hist = a.scratch + s;
  double* const Cw = hist + (size_t)a.T * 2 * SLOT * ld;
  double* const Dw = Cw + (size_t)(N * N) * ld;
  for (int t = a.T - 1; t >= 0; --t) {
    const size_t f = (size_t)s * a.T + t;
    double* F0 = hist + (size_t)(t * 2) * SLOT * ld;
    const bool est = a.flags[f] != KFN_POSE_NONE;
    if (t + 1 < a.T && est && a.flags[f + 1] != KFN_POSE_INIT)
      smooth_step<N>(F0, F0 + (size_t)2 * SLOT * ld, F0 + (size_t)3 * SLOT * ld, Cw, Dw, ld);
    float* op = a.smooth_poses + f * 16;
    float* oc = a.smooth_cov + f * 36;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) op[r * 4 + c] = est ? (float)F0[(size_t)(r * 3 + c) * ld] : __builtin_nanf("");
      op[r * 4 + 3] = est ? (float)F0[(size_t)(9 + r) * ld] : __builtin_nanf("");
    }
    for (int c = 0; c < 4; ++c) op[12 + c] = est ? ((c == 3) ? 1.f : 0.f) : __builtin_nanf("");
    for (int i = 0; i < 36; ++i) oc[i] = est ? (float)F0[(size_t)(OFF_P + (i / 6) * N + i % 6) * ld] : __builtin_nanf("");
  }
}

#undef P12

// The checks of the descriptor that the three entry points share.
int check_desc(const kfn_pose_track_desc* desc, const char* who, kfn_pose_track_desc* out) {
  if (desc == nullptr) return kfn::fail(KFN_ERR_ARG, "%s: null descriptor", who);
  if (desc->struct_size < (int32_t)sizeof(kfn_pose_track_desc) || (desc->struct_size & 3) != 0)
    return kfn::fail(KFN_ERR_ARG, "%s: kfn_pose_track_desc.struct_size = %d (this library: %d bytes) -- use "
                     "KFN_POSE_TRACK_DESC_INIT", who, (int)desc->struct_size, (int)sizeof(kfn_pose_track_desc));
  const kfn_pose_track_desc d = *desc;
  KFN_REQUIRE(d.S > 0 && d.T > 0 && (long)d.S * d.T <= (1L << 24), "%s: bad shape S=%d T=%d", who, d.S, d.T);
  KFN_REQUIRE(d.model == KFN_POSE_MODEL_WALK || d.model == KFN_POSE_MODEL_VELOCITY, "%s: model = %d (KFN_POSE_MODEL_WALK or "
              "KFN_POSE_MODEL_VELOCITY)", who, d.model);
  KFN_REQUIRE(d.smooth == 0 || d.smooth == 1, "%s: smooth = %d (0 or 1)", who, d.smooth);
  KFN_REQUIRE(d.rot_sigma >= 0.f && d.trans_sigma >= 0.f && std::isfinite(d.rot_sigma) && std::isfinite(d.trans_sigma),
              "%s: rot_sigma = %g, trans_sigma = %g (>= 0)", who, (double)d.rot_sigma, (double)d.trans_sigma);
  if (d.model == KFN_POSE_MODEL_VELOCITY)
    KFN_REQUIRE(d.rot_rate_sigma > 0.f && d.trans_rate_sigma > 0.f && std::isfinite(d.rot_rate_sigma) &&
                std::isfinite(d.trans_rate_sigma), "%s: rot_rate_sigma = %g, trans_rate_sigma = %g (> 0 under the velocity model)",
                who, (double)d.rot_rate_sigma, (double)d.trans_rate_sigma);
  KFN_REQUIRE(d.gate > 0.f && !std::isnan(d.gate), "%s: gate = %g (> 0)", who, (double)d.gate);
  KFN_REQUIRE(d.max_rejects >= 1, "%s: max_rejects = %d < 1", who, d.max_rejects);
  *out = d;
  return KFN_OK;
}

size_t state_doubles(const kfn_pose_track_desc& d) {
  return (size_t)d.S * (2 + slot_doubles(d.model == KFN_POSE_MODEL_VELOCITY ? 12 : 6));
}

size_t scratch_doubles(const kfn_pose_track_desc& d) {
  if (!d.smooth) return 0;
  const int n = d.model == KFN_POSE_MODEL_VELOCITY ? 12 : 6;
  return (size_t)d.S * ((size_t)d.T * 2 * slot_doubles(n) + 2 * n * n);
}

}  // namespace

extern "C" int kfn_pose_track_state_bytes(const kfn_pose_track_desc* desc, size_t* bytes) {
  kfn_pose_track_desc d;
  if (int rc = check_desc(desc, "kfn_pose_track_state_bytes", &d)) return rc;
  KFN_REQUIRE(bytes, "kfn_pose_track_state_bytes: null argument");
  *bytes = state_doubles(d) * sizeof(double);
  return KFN_OK;
}

extern "C" int kfn_pose_track_scratch_bytes(const kfn_pose_track_desc* desc, size_t* bytes) {
  kfn_pose_track_desc d;
  if (int rc = check_desc(desc, "kfn_pose_track_scratch_bytes", &d)) return rc;
  KFN_REQUIRE(bytes, "kfn_pose_track_scratch_bytes: null argument");
  *bytes = scratch_doubles(d) * sizeof(double);
  return KFN_OK;
}

extern "C" int kfn_pose_track(const kfn_pose_track_desc* desc, const float* poses, const float* cov, void* state,
                              float* out_poses, float* out_cov, int32_t* flags, float* nis, float* smooth_poses,
                              float* smooth_cov, void* scratch, void* stream) {
  kfn_pose_track_desc d;
  if (int rc = check_desc(desc, "kfn_pose_track", &d)) return rc;
  KFN_REQUIRE(poses && cov && out_poses && out_cov && flags && nis, "kfn_pose_track: null argument");
  if (d.smooth)
    KFN_REQUIRE(smooth_poses && smooth_cov && scratch, "kfn_pose_track: smooth = 1 needs smooth_poses, smooth_cov and scratch "
                "(kfn_pose_track_scratch_bytes)");
  else
    KFN_REQUIRE(!smooth_poses && !smooth_cov, "kfn_pose_track: smooth = 0, but a smoothed output is given");
  KFN_REQUIRE(((uintptr_t)state & 7) == 0 && ((uintptr_t)scratch & 7) == 0, "kfn_pose_track: state and scratch must be "
              "aligned to 8 bytes");
  TrackArgs a;
  a.poses = poses; a.cov = cov; a.state = (double*)state; a.out_poses = out_poses; a.out_cov = out_cov; a.flags = flags;
  a.nis = nis; a.smooth_poses = smooth_poses; a.smooth_cov = smooth_cov; a.scratch = d.smooth ? (double*)scratch : nullptr;
  a.S = d.S; a.T = d.T; a.max_rejects = d.max_rejects; a.smooth = d.smooth;
  a.qr = (double)d.rot_sigma * (double)d.rot_sigma;
  a.qt = (double)d.trans_sigma * (double)d.trans_sigma;
  a.gate = (double)d.gate;
  a.rr = (double)d.rot_rate_sigma * (double)d.rot_rate_sigma;
  a.rt = (double)d.trans_rate_sigma * (double)d.trans_rate_sigma;
  const dim3 grid((unsigned)kfn::ceil_div(d.S, LANES));
  if (d.model == KFN_POSE_MODEL_VELOCITY) {
    auto kern = pose_track_kernel<12>;
    static std::atomic<uint64_t> attr_done{0};
    if (int rc = kfn::set_max_dynamic_lds(reinterpret_cast<const void*>(kern), P12_LDS_BYTES, attr_done)) return rc;
    hipLaunchKernelGGL(kern, grid, dim3(LANES), P12_LDS_BYTES, (hipStream_t)stream, a);
    KFN_LAUNCH_CHECK("pose_track_kernel");
    if (d.smooth) hipLaunchKernelGGL(pose_smooth_kernel<12>, grid, dim3(LANES), 0, (hipStream_t)stream, a);
  } else {
    hipLaunchKernelGGL(pose_track_kernel<6>, grid, dim3(LANES), 0, (hipStream_t)stream, a);
    KFN_LAUNCH_CHECK("pose_track_kernel");
    if (d.smooth) hipLaunchKernelGGL(pose_smooth_kernel<6>, grid, dim3(LANES), 0, (hipStream_t)stream, a);
  }
  KFN_LAUNCH_CHECK("pose_smooth_kernel");
  return KFN_OK;
}
