// kfn_pose_filter.hip -- a random-walk error-state Kalman filter over the per-frame camera poses of kfn_pnp_ransac_unc.
//
// One sequence per lane, fp64, serial over t (the shape of the Kalman scan: a sequence is a chain, sequences are
// independent).  State: (R, p) camera-to-world and P, the 6x6 covariance of the body-frame perturbation (dtheta, drho),
// C ~ C_hat [exp(dtheta) | drho] -- the coordinates kfn_pnp_ransac_unc's cov is given in.  DESIGN.md 5c "Uncertainty" fixes
// every step, and tests/pnp_unc_ref.py restates them in numpy; built with -ffp-contract=off so that the restatement rounds
// the same products and sums.
//
// Approximation: the innovation covariance S = P + Sigma_z adds two covariances that are expressed in two body frames (the
// state's and the measurement's); the rotation between them, which is of the size of the innovation itself, is neglected.
#include <cmath>

#include "kfn_common.h"

namespace {

constexpr int LANES = 64;

struct FilterArgs {
  const float* poses;
  const float* cov;
  float* out_poses;
  float* out_cov;
  int* flags;
  float* nis;
  int S, T, max_rejects;
  double qr, qt, gate;   // rot_sigma^2, trans_sigma^2, the NIS gate
};

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

// grid (ceil(S / 64)), 64 threads: lane = sequence
__global__ __launch_bounds__(LANES) void pose_filter_kernel(FilterArgs a) {
  const int s = blockIdx.x * LANES + threadIdx.x;
  if (s >= a.S) return;
  const double nan = __builtin_nan("");
  bool have = false;
  int rejects = 0;
  double R[9], p[3], P[6][6];
  for (int t = 0; t < a.T; ++t) {
    const size_t f = (size_t)s * a.T + t;
    const float* z = a.poses + f * 16;
    const float* cz = a.cov + f * 36;
    bool valid = true;
    for (int i = 0; i < 12; ++i) valid = valid && isfinite(z[i]);
    for (int i = 0; i < 36; ++i) valid = valid && isfinite(cz[i]);
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
      for (int i = 0; i < 6; ++i) P[i][i] += (i < 3) ? a.qr : a.qt;
      flag = KFN_POSE_MISSING;
      if (valid) {
        // innovation y = (log(R^T R_z), R^T (p_z - p)), S = P + Sigma_z = L L^T
        double M[9], y[6], L[6][6], u[6];
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 3; ++c) M[r * 3 + c] = R[0 * 3 + r] * Rz[0 * 3 + c] + R[1 * 3 + r] * Rz[1 * 3 + c] + R[2 * 3 + r] * Rz[2 * 3 + c];
        log_so3(M, y);
        const double dp[3] = {pz[0] - p[0], pz[1] - p[1], pz[2] - p[2]};
        for (int r = 0; r < 3; ++r) y[3 + r] = R[0 * 3 + r] * dp[0] + R[1 * 3 + r] * dp[1] + R[2 * 3 + r] * dp[2];
        for (int i = 0; i < 6; ++i)
          for (int j = 0; j < 6; ++j) L[i][j] = P[i][j] + (double)cz[i * 6 + j];
        if (chol6(L)) {
          forward6(L, y, u);
          nisv = 0.0;
          for (int i = 0; i < 6; ++i) nisv += u[i] * u[i];
          if (nisv > a.gate) {
            ++rejects;
            flag = KFN_POSE_REJECTED;
            if (rejects >= a.max_rejects) { flag = KFN_POSE_INIT; init = true; }
          } else {
            // K = P S^-1 row by row (S and P symmetric: row i of K solves S k = P[i,:]); delta = K y
            double K[6][6], d[6], A[6][6], AP[6][6], KS[6][6];
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
            for (int i = 0; i < 6; ++i)
              for (int j = 0; j < 6; ++j) {
                double s1 = 0.0, s2 = 0.0;
                for (int k = 0; k < 6; ++k) { s1 += A[i][k] * P[k][j]; s2 += K[i][k] * (double)cz[k * 6 + j]; }
                AP[i][j] = s1;
                KS[i][j] = s2;
              }
            for (int i = 0; i < 6; ++i)
              for (int j = i; j < 6; ++j) {
                double s1 = 0.0, s2 = 0.0;
                for (int k = 0; k < 6; ++k) { s1 += AP[i][k] * A[j][k]; s2 += KS[i][k] * K[j][k]; }
                P[i][j] = s1 + s2;
                P[j][i] = s1 + s2;
              }
            flag = KFN_POSE_UPDATED;
            rejects = 0;
          }
        }
      }
    }
    if (init) {
      for (int i = 0; i < 9; ++i) R[i] = Rz[i];
      for (int i = 0; i < 3; ++i) p[i] = pz[i];
      for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) P[i][j] = (double)cz[i * 6 + j];
      have = true;
      rejects = 0;
    }
    float* op = a.out_poses + f * 16;
    float* oc = a.out_cov + f * 36;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) op[r * 4 + c] = have ? (float)R[r * 3 + c] : __builtin_nanf("");
      op[r * 4 + 3] = have ? (float)p[r] : __builtin_nanf("");
    }
    for (int c = 0; c < 4; ++c) op[12 + c] = have ? ((c == 3) ? 1.f : 0.f) : __builtin_nanf("");
    for (int i = 0; i < 36; ++i) oc[i] = have ? (float)P[i / 6][i % 6] : __builtin_nanf("");
    a.flags[f] = flag;
    a.nis[f] = (float)nisv;
  }
}

}  // namespace

extern "C" int kfn_pose_filter(const kfn_pose_filter_desc* desc, const float* poses, const float* cov, float* out_poses,
                               float* out_cov, int32_t* flags, float* nis, void* stream) {
  if (desc == nullptr) return kfn::fail(KFN_ERR_ARG, "kfn_pose_filter: null descriptor");
  if (desc->struct_size < (int32_t)sizeof(kfn_pose_filter_desc) || (desc->struct_size & 3) != 0)
    return kfn::fail(KFN_ERR_ARG, "kfn_pose_filter: kfn_pose_filter_desc.struct_size = %d (this library: %d bytes) -- use "
                     "KFN_POSE_FILTER_DESC_INIT", (int)desc->struct_size, (int)sizeof(kfn_pose_filter_desc));
  const kfn_pose_filter_desc d = *desc;
  KFN_REQUIRE(d.S > 0 && d.T > 0 && (long)d.S * d.T <= (1L << 24), "kfn_pose_filter: bad shape S=%d T=%d", d.S, d.T);
  KFN_REQUIRE(d.rot_sigma >= 0.f && d.trans_sigma >= 0.f && std::isfinite(d.rot_sigma) && std::isfinite(d.trans_sigma),
              "kfn_pose_filter: rot_sigma = %g, trans_sigma = %g (>= 0)", (double)d.rot_sigma, (double)d.trans_sigma);
  KFN_REQUIRE(d.gate > 0.f && !std::isnan(d.gate), "kfn_pose_filter: gate = %g (> 0)", (double)d.gate);
  KFN_REQUIRE(d.max_rejects >= 1, "kfn_pose_filter: max_rejects = %d < 1", d.max_rejects);
  KFN_REQUIRE(poses && cov && out_poses && out_cov && flags && nis, "kfn_pose_filter: null argument");
  FilterArgs a;
  a.poses = poses; a.cov = cov; a.out_poses = out_poses; a.out_cov = out_cov; a.flags = flags; a.nis = nis;
  a.S = d.S; a.T = d.T; a.max_rejects = d.max_rejects;
  a.qr = (double)d.rot_sigma * (double)d.rot_sigma;
  a.qt = (double)d.trans_sigma * (double)d.trans_sigma;
  a.gate = (double)d.gate;
  hipLaunchKernelGGL(pose_filter_kernel, dim3((unsigned)kfn::ceil_div(d.S, LANES)), dim3(LANES), 0, (hipStream_t)stream, a);
  KFN_LAUNCH_CHECK("pose_filter_kernel");
  return KFN_OK;
}
