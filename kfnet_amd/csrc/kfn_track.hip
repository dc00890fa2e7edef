// kfn_track.hip -- the camera tracked against the TSDF volume of kfn_fuse.hip (gfx950): live vertex and normal maps from a
// depth map, the model's maps by ray casting, the sums of projective point-to-plane ICP, the 6x6 solve and the commit.
// Compiled with -ffp-contract=off: every fp32 line below is one rounded operation of include/kfnet_hip.h (the kfn_track_*
// block), in that order, so the numpy float32 restatement (tests/track_ref.py) gives the same bits for the maps and the
// per-pixel rows.  Quotients and square roots are IEEE (hipcc's default for fp32).  The 29 sums are fp64 over a fixed tree;
// there is no floating-point atomic and no workgroup waits for another.
//
//   maps         [sum_l H_l W_l] quadruples, level l at offset sum_{k<l} H_k W_k, row-major; (x, y, z, 1) valid, zeros invalid.
//   level l      H_l = H_{l-1} / 2, W_l = W_{l-1} / 2 (floor); fx_l = fx_{l-1} 0.5, cu_l = (cu_{l-1} - 0.5) 0.5, likewise fy, cv.
//   record       kfn_track_state: committed pose and estimate as 12 doubles [R|t] row-major, camera to world.
#include "kfn_common.h"
#include <cfloat>
#include <cmath>

namespace {

constexpr int TT = 256;                    // threads of a workgroup of the per-pixel kernels
constexpr int ICP_ITEMS = 4;               // pixels a thread of the ICP kernel takes
constexpr int ICP_BLOCK = TT * ICP_ITEMS;
constexpr int SUMS = 29, SUMS_LD = 32;     // the sums and the doubles a row of partials takes
constexpr int MAX_LEVELS = 4;
constexpr int MAX_STEPS = 8191;            // the largest sample index of a ray
constexpr int TRAJ_LD = 20;                // doubles a trajectory row takes

struct Level {
  int H, W;
  long off;                                // quadruples before this level
  float fx, fy, cu, cv;
};

struct RayArgs {
  const float2* tsdf;
  const kfn_track_state* state;
  float4* mv;
  float4* mn;
  Level lv;
  int nx, ny, nz;
  float ox, oy, oz, voxel, half_trunc, near, far, min_weight;
};

struct IcpArgs {
  const float4* lv;
  const float4* ln;
  const float4* mv;
  const float4* mn;
  const kfn_track_state* state;
  double* partial;
  Level lvl;
  float near, dist_max, cos_min;
};

__device__ __forceinline__ bool finite(float x) { return fabsf(x) <= FLT_MAX; }

// ---- live maps ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TT) void track_vertex0_kernel(const uint16_t* depth, float4* out, Level lv, int raw_min, int raw_max,
                                                           float scale) {
  const int i = blockIdx.x * TT + threadIdx.x;
  if (i >= lv.H * lv.W) return;
  const int x = i % lv.W, y = i / lv.W;
  const int raw = (int)depth[i];
  float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (raw >= raw_min && raw <= raw_max) {
    const float z = (float)raw * scale;
    v.x = (((float)x - lv.cu) / lv.fx) * z;
    v.y = (((float)y - lv.cv) / lv.fy) * z;
    v.z = z;
    v.w = 1.0f;
  }
  out[i] = v;
}

// dst pixel (x, y) from the src block (2x, 2y) .. (2x + 1, 2y + 1), which lies inside src because dst is floor(src / 2)
__global__ __launch_bounds__(TT) void track_pyramid_kernel(const float4* src, float4* dst, int Ws, Level lv, float pyr_dist) {
  const int i = blockIdx.x * TT + threadIdx.x;
  if (i >= lv.H * lv.W) return;
  const int x = i % lv.W, y = i / lv.W;
  float z[4];
  bool ok[4];
  float zmin = FLT_MAX;
  bool any = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float4 s = src[(long)(2 * y + (k >> 1)) * Ws + (2 * x + (k & 1))];
    z[k] = s.z;
    ok[k] = s.w != 0.0f;
    if (ok[k]) {
      zmin = fminf(zmin, s.z);
      any = true;
    }
  }
  float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (any) {
    float sum = 0.0f, cnt = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (ok[k] && z[k] - zmin <= pyr_dist) {
        sum = sum + z[k];
        cnt = cnt + 1.0f;
      }
    }
    const float zz = sum / cnt;
    v.x = (((float)x - lv.cu) / lv.fx) * zz;
    v.y = (((float)y - lv.cv) / lv.fy) * zz;
    v.z = zz;
    v.w = 1.0f;
  }
  dst[i] = v;
}

__global__ __launch_bounds__(TT) void track_normal_kernel(const float4* vm, float4* nm, int H, int W, float jump) {
  const int i = blockIdx.x * TT + threadIdx.x;
  if (i >= H * W) return;
  const int x = i % W, y = i / W;
  float4 n = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (x + 1 < W && y + 1 < H) {
    const float4 v = vm[i], r = vm[i + 1], d = vm[i + W];
    if (v.w != 0.0f && r.w != 0.0f && d.w != 0.0f && fabsf(r.z - v.z) <= jump && fabsf(d.z - v.z) <= jump) {
      const float ax = d.x - v.x, ay = d.y - v.y, az = d.z - v.z;           // to the lower neighbour
      const float bx = r.x - v.x, by = r.y - v.y, bz = r.z - v.z;           // to the right neighbour
      const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
      const float len = sqrtf((cx * cx + cy * cy) + cz * cz);
      if (len > 0.0f && finite(len)) n = make_float4(cx / len, cy / len, cz / len, 1.0f);
    }
  }
  nm[i] = n;
}

// ---- the ray cast -------------------------------------------------------------------------------------------------------------
// The trilinear D at lattice coordinates g.  Usable iff floor(g) lies in 0 .. n-2 on every axis, compared in float before the
// conversion (a NaN fails every comparison), and all eight points around it have W >= min_weight.
__device__ __forceinline__ bool sample(const RayArgs& p, float gx, float gy, float gz, float* D) {
  const float x0 = floorf(gx), y0 = floorf(gy), z0 = floorf(gz);
  if (!(x0 >= 0.0f && x0 <= (float)(p.nx - 2) && y0 >= 0.0f && y0 <= (float)(p.ny - 2) && z0 >= 0.0f && z0 <= (float)(p.nz - 2)))
    return false;
  const long sy = p.nx, sz = (long)p.nx * p.ny;
  const float2* q = p.tsdf + ((long)(int)z0 * p.ny + (int)y0) * p.nx + (int)x0;
  const float2 d000 = q[0], d100 = q[1], d010 = q[sy], d110 = q[sy + 1];
  const float2 d001 = q[sz], d101 = q[sz + 1], d011 = q[sz + sy], d111 = q[sz + sy + 1];
  const float w = p.min_weight;
  if (!(d000.y >= w && d100.y >= w && d010.y >= w && d110.y >= w && d001.y >= w && d101.y >= w && d011.y >= w && d111.y >= w))
    return false;
  const float a = gx - x0, b = gy - y0, c = gz - z0;
  const float c00 = d000.x + a * (d100.x - d000.x);
  const float c10 = d010.x + a * (d110.x - d010.x);
  const float c01 = d001.x + a * (d101.x - d001.x);
  const float c11 = d011.x + a * (d111.x - d011.x);
  const float c0 = c00 + b * (c10 - c00);
  const float c1 = c01 + b * (c11 - c01);
  *D = c0 + c * (c1 - c0);
  return true;
}

__global__ __launch_bounds__(TT) void track_raycast_kernel(RayArgs p) {
  const int i = blockIdx.x * TT + threadIdx.x;
  if (i >= p.lv.H * p.lv.W) return;
  const int x = i % p.lv.W, y = i / p.lv.W;
  float P[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) P[k] = (float)p.state->committed[k];
  float4 vout = make_float4(0.0f, 0.0f, 0.0f, 0.0f), nout = vout;
  const float qx = ((float)x - p.lv.cu) / p.lv.fx, qy = ((float)y - p.lv.cv) / p.lv.fy;
  const float wx = (P[0] * qx + P[1] * qy) + P[2];             // the ray's direction, z-depth 1 per unit of t
  const float wy = (P[4] * qx + P[5] * qy) + P[6];
  const float wz = (P[8] * qx + P[9] * qy) + P[10];
  const float len = sqrtf((qx * qx + qy * qy) + 1.0f);
  const float dt = p.half_trunc / len;
  const float gcx = (P[3] - p.ox) / p.voxel, gcy = (P[7] - p.oy) / p.voxel, gcz = (P[11] - p.oz) / p.voxel;
  const float gdx = wx / p.voxel, gdy = wy / p.voxel, gdz = wz / p.voxel;
  // slab test against the lattice's box 0 .. n-1
  float tmin = p.near, tmax = p.far;
  {
    const float ix = 1.0f / gdx, iy = 1.0f / gdy, iz = 1.0f / gdz;
    const float ax = (0.0f - gcx) * ix, bx = ((float)(p.nx - 1) - gcx) * ix;
    const float ay = (0.0f - gcy) * iy, by = ((float)(p.ny - 1) - gcy) * iy;
    const float az = (0.0f - gcz) * iz, bz = ((float)(p.nz - 1) - gcz) * iz;
    tmin = fmaxf(tmin, fminf(ax, bx)); tmax = fminf(tmax, fmaxf(ax, bx));
    tmin = fmaxf(tmin, fminf(ay, by)); tmax = fminf(tmax, fmaxf(ay, by));
    tmin = fmaxf(tmin, fminf(az, bz)); tmax = fminf(tmax, fmaxf(az, bz));
  }
  const float kf = floorf((tmax - tmin) / dt);
  bool sane = true;
#pragma unroll
  for (int k = 0; k < 12; ++k) sane = sane && finite(P[k]);
  if (sane && tmin < tmax && kf >= 0.0f) {
    const int kmax = (int)fminf(kf, (float)MAX_STEPS);
    bool positive = false, hit = false;
    float Dp = 0.0f, tp = 0.0f, Dc = 0.0f, tc = 0.0f;
    for (int k = 0; k <= kmax; ++k) {
      const float t = tmin + (float)k * dt;
      float D;
      if (!sample(p, gcx + t * gdx, gcy + t * gdy, gcz + t * gdz, &D)) {
        positive = false;
        continue;
      }
      if (D > 0.0f) {
        positive = true;
        Dp = D;
        tp = t;
        continue;
      }
      if (D < 0.0f) {                       // the surface if it follows a usable D > 0; otherwise a back face or unknown: invalid
        hit = positive;
        Dc = D;
        tc = t;
        break;
      }
      positive = false;                     // D == 0 or NaN
    }
    if (hit) {
      const float ts = tp + (Dp / (Dp - Dc)) * (tc - tp);
      vout = make_float4(P[3] + ts * wx, P[7] + ts * wy, P[11] + ts * wz, 1.0f);
      const float gx = gcx + ts * gdx, gy = gcy + ts * gdy, gz = gcz + ts * gdz;
      float xp, xm, yp, ym, zp, zm;
      if (sample(p, gx + 1.0f, gy, gz, &xp) && sample(p, gx - 1.0f, gy, gz, &xm) && sample(p, gx, gy + 1.0f, gz, &yp) &&
          sample(p, gx, gy - 1.0f, gz, &ym) && sample(p, gx, gy, gz + 1.0f, &zp) && sample(p, gx, gy, gz - 1.0f, &zm)) {
        const float nx = xp - xm, ny = yp - ym, nz = zp - zm;
        const float nl = sqrtf((nx * nx + ny * ny) + nz * nz);
        if (nl > 0.0f && finite(nl)) nout = make_float4(nx / nl, ny / nl, nz / nl, 1.0f);
      }
    }
  }
  p.mv[p.lv.off + i] = vout;
  p.mn[p.lv.off + i] = nout;
}

// ---- the ICP sums -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}

__global__ __launch_bounds__(TT) void track_icp_kernel(IcpArgs p) {
  __shared__ double wave_part[TT / 64][SUMS_LD];
  const int tid = threadIdx.x;
  const int pixels = p.lvl.H * p.lvl.W;
  float E[12], Cm[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    E[k] = (float)p.state->estimate[k];
    Cm[k] = (float)p.state->committed[k];
  }
  const float wmax = (float)(p.lvl.W - 1), hmax = (float)(p.lvl.H - 1);
  double acc[SUMS];
#pragma unroll
  for (int k = 0; k < SUMS; ++k) acc[k] = 0.0;
  for (int j = 0; j < ICP_ITEMS; ++j) {
    const int i = blockIdx.x * ICP_BLOCK + j * TT + tid;
    if (i >= pixels) continue;
    const float4 v = p.lv[p.lvl.off + i], nl = p.ln[p.lvl.off + i];
    if (v.w == 0.0f || nl.w == 0.0f) continue;
    const float px = ((E[0] * v.x + E[1] * v.y) + E[2] * v.z) + E[3];
    const float py = ((E[4] * v.x + E[5] * v.y) + E[6] * v.z) + E[7];
    const float pz = ((E[8] * v.x + E[9] * v.y) + E[10] * v.z) + E[11];
    const float dx = px - Cm[3], dy = py - Cm[7], dz = pz - Cm[11];
    const float X = (Cm[0] * dx + Cm[4] * dy) + Cm[8] * dz;
    const float Y = (Cm[1] * dx + Cm[5] * dy) + Cm[9] * dz;
    const float Z = (Cm[2] * dx + Cm[6] * dy) + Cm[10] * dz;
    if (!(finite(X) && finite(Y) && finite(Z)) || Z < p.near) continue;
    const float cf = rintf((X / Z) * p.lvl.fx + p.lvl.cu), rf = rintf((Y / Z) * p.lvl.fy + p.lvl.cv);
    if (!(cf >= 0.0f && cf <= wmax && rf >= 0.0f && rf <= hmax)) continue;
    const long at = p.lvl.off + (long)(int)rf * p.lvl.W + (int)cf;
    const float4 m = p.mv[at], n = p.mn[at];
    if (m.w == 0.0f || n.w == 0.0f) continue;
    const float ex = m.x - px, ey = m.y - py, ez = m.z - pz;
    const float dist = sqrtf((ex * ex + ey * ey) + ez * ez);
    if (!(dist <= p.dist_max)) continue;
    const float rx = (E[0] * nl.x + E[1] * nl.y) + E[2] * nl.z;
    const float ry = (E[4] * nl.x + E[5] * nl.y) + E[6] * nl.z;
    const float rz = (E[8] * nl.x + E[9] * nl.y) + E[10] * nl.z;
    const float dot = (rx * n.x + ry * n.y) + rz * n.z;
    if (!(dot >= p.cos_min)) continue;
    const float r = (n.x * ex + n.y * ey) + n.z * ez;
    float J[6];
    J[0] = py * n.z - pz * n.y;
    J[1] = pz * n.x - px * n.z;
    J[2] = px * n.y - py * n.x;
    J[3] = n.x; J[4] = n.y; J[5] = n.z;
    // products of two floats are exact in fp64
    int s = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
      for (int b = a; b < 6; ++b) {
        acc[s] = acc[s] + (double)J[a] * (double)J[b];
        ++s;
      }
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) acc[21 + a] = acc[21 + a] + (double)J[a] * (double)r;
    acc[27] = acc[27] + (double)r * (double)r;
    acc[28] = acc[28] + 1.0;
  }
  const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int k = 0; k < SUMS; ++k) {
    const double s = wave_sum_f64(acc[k]);
    if (lane == 0) wave_part[wave][k] = s;
  }
  __syncthreads();
  if (tid < SUMS_LD) {
    double s = 0.0;
    if (tid < SUMS) s = (wave_part[0][tid] + wave_part[1][tid]) + (wave_part[2][tid] + wave_part[3][tid]);
    p.partial[(long)blockIdx.x * SUMS_LD + tid] = s;
  }
}

__global__ __launch_bounds__(64) void track_reduce_kernel(const double* partial, int blocks, double* sums) {
  const int k = threadIdx.x;
  if (k >= SUMS_LD) return;
  double s = 0.0;
  for (int b = 0; b < blocks; ++b) s = s + partial[(long)b * SUMS_LD + k];
  sums[k] = s;
}

// ---- solve and commit -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool finite64(double x) { return fabs(x) <= DBL_MAX; }

// c0 = col0 / |col0|; c1 = col1 - (c0 . col1) c0, normalised; c2 = c0 x c1.  R is row-major 3 x 3 inside the 3 x 4 pose.
__device__ void orthonormalise(double* P) {
  double a0 = P[0], a1 = P[4], a2 = P[8], b0 = P[1], b1 = P[5], b2 = P[9];
  const double la = sqrt((a0 * a0 + a1 * a1) + a2 * a2);
  a0 = a0 / la; a1 = a1 / la; a2 = a2 / la;
  const double d = (a0 * b0 + a1 * b1) + a2 * b2;
  b0 = b0 - d * a0; b1 = b1 - d * a1; b2 = b2 - d * a2;
  const double lb = sqrt((b0 * b0 + b1 * b1) + b2 * b2);
  b0 = b0 / lb; b1 = b1 / lb; b2 = b2 / lb;
  P[0] = a0; P[4] = a1; P[8] = a2;
  P[1] = b0; P[5] = b1; P[9] = b2;
  P[2] = a1 * b2 - a2 * b1;
  P[6] = a2 * b0 - a0 * b2;
  P[10] = a0 * b1 - a1 * b0;
}

__global__ __launch_bounds__(64) void track_update_kernel(const double* sums, kfn_track_state* st, int pixels, int min_pairs,
                                                          double pivot_floor) {
  if (threadIdx.x != 0) return;
  const double count = sums[28];
  st->last_pairs = count;
  st->last_share = count / (double)pixels;
  st->last_rms = count > 0.0 ? sqrt(sums[27] / count) : 0.0;
  st->iterations = st->iterations + 1;
  if (!(count >= (double)min_pairs)) return;
  double A[6][6], L[6][6], b[6], y[6], xi[6];
  {
    int s = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
      for (int j = i; j < 6; ++j) {
        A[i][j] = sums[s];
        A[j][i] = sums[s];
        ++s;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) b[i] = sums[21 + i];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = A[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d = d - L[j][k] * L[j][k];
    if (!(d > pivot_floor * A[j][j]) || !finite64(d)) ok = false;
    const double l = sqrt(ok ? d : 1.0);
    L[j][j] = l;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double s = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) s = s - L[i][k] * L[j][k];
      L[i][j] = s / l;
    }
  }
  if (!ok) return;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
    y[i] = s / L[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double s = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) s = s - L[k][i] * xi[k];
    xi[i] = s / L[i][i];
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) ok = ok && finite64(xi[i]);
  if (!ok) return;
  // exp of the twist (w, u): R = I + A K + B K^2, t = (I + B K + C K^2) u with K = [w]x, theta = |w|
  const double w0 = xi[0], w1 = xi[1], w2 = xi[2];
  const double th2 = (w0 * w0 + w1 * w1) + w2 * w2;
  const double th = sqrt(th2);
  double Ac, Bc, Cc;
  if (th < 1e-4) {
    Ac = 1.0 - th2 / 6.0;
    Bc = 0.5 - th2 / 24.0;
    Cc = 1.0 / 6.0 - th2 / 120.0;
  } else {
    const double sh = sin(0.5 * th);
    Ac = sin(th) / th;
    Bc = (2.0 * sh * sh) / th2;
    Cc = (1.0 - Ac) / th2;
  }
  const double K[9] = {0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0};
  double K2[9], Ri[9], V[9];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) K2[3 * i + j] = (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j]) + K[3 * i + 2] * K[6 + j];
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const double id = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
    Ri[k] = (id + Ac * K[k]) + Bc * K2[k];
    V[k] = (id + Bc * K[k]) + Cc * K2[k];
  }
  double ti[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) ti[i] = (V[3 * i] * xi[3] + V[3 * i + 1] * xi[4]) + V[3 * i + 2] * xi[5];
  double E[12], N[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) E[k] = st->estimate[k];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) N[4 * i + j] = (Ri[3 * i] * E[j] + Ri[3 * i + 1] * E[4 + j]) + Ri[3 * i + 2] * E[8 + j];
    N[4 * i + 3] = N[4 * i + 3] + ti[i];
  }
  orthonormalise(N);
#pragma unroll
  for (int k = 0; k < 12; ++k) ok = ok && finite64(N[k]);
  if (!ok) return;
#pragma unroll
  for (int k = 0; k < 12; ++k) st->estimate[k] = N[k];
  st->accepted = st->accepted + 1;
}

__global__ __launch_bounds__(64) void track_commit_kernel(kfn_track_state* st, float* pose_row, double* trajectory, int traj_rows,
                                                          double min_share, double max_rms, double max_step_m, double max_step_rad) {
  if (threadIdx.x != 0) return;
  double E[12], Cm[12];
  bool fin = true;
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    E[k] = st->estimate[k];
    Cm[k] = st->committed[k];
    fin = fin && finite64(E[k]);
  }
  const double dx = E[3] - Cm[3], dy = E[7] - Cm[7], dz = E[11] - Cm[11];
  const double step_m = sqrt((dx * dx + dy * dy) + dz * dz);
  double tr = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) tr = tr + E[4 * i + j] * Cm[4 * i + j];
  }
  const double step_rad = acos(fmin(fmax((tr - 1.0) * 0.5, -1.0), 1.0));
  const bool tracked = fin && st->accepted > 0 && st->last_share >= min_share && st->last_rms <= max_rms &&
                       step_m <= max_step_m && step_rad <= max_step_rad;
  const double nan = __builtin_nan("");
  const int row = st->frame;
  if (tracked) {
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      st->committed[k] = E[k];
      pose_row[k] = (float)E[k];
    }
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      st->estimate[k] = Cm[k];
      pose_row[k] = __builtin_nanf("");
    }
    st->lost = st->lost + 1;
  }
  if (row >= 0 && row < traj_rows) {
    double* t = trajectory + (long)row * TRAJ_LD;
#pragma unroll
    for (int k = 0; k < 12; ++k) t[k] = tracked ? E[k] : nan;
    t[12] = tracked ? 0.0 : 1.0;
    t[13] = st->last_pairs;
    t[14] = st->last_share;
    t[15] = st->last_rms;
    t[16] = (double)st->accepted;
    t[17] = (double)st->iterations;
    t[18] = step_m;
    t[19] = step_rad;
  }
  st->frame = row + 1;
  st->accepted = 0;
  st->iterations = 0;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
bool host_finite(float x) { return x - x == 0.0f; }

Level level_of(const kfn_track_desc* d, int l) {
  Level lv;
  lv.H = d->H; lv.W = d->W; lv.off = 0;
  lv.fx = d->dfx; lv.fy = d->dfy; lv.cu = d->du; lv.cv = d->dv;
  for (int k = 0; k < l; ++k) {
    lv.off += (long)lv.H * lv.W;
    lv.H /= 2; lv.W /= 2;
    lv.fx = lv.fx * 0.5f; lv.fy = lv.fy * 0.5f;
    lv.cu = (lv.cu - 0.5f) * 0.5f; lv.cv = (lv.cv - 0.5f) * 0.5f;
  }
  return lv;
}

int checked_track(const kfn_track_desc* d, const char* who) {
  KFN_REQUIRE(d, "%s: null descriptor", who);
  KFN_REQUIRE(d->struct_size == (int32_t)sizeof(kfn_track_desc), "%s: struct_size %d, expected %d", who, (int)d->struct_size,
              (int)sizeof(kfn_track_desc));
  KFN_REQUIRE(d->H > 0 && d->W > 0 && (long)d->H * d->W < (1L << 28), "%s: the image size must be positive and below 2^28 pixels (%dx%d)",
              who, d->H, d->W);
  KFN_REQUIRE(d->levels >= 1 && d->levels <= MAX_LEVELS, "%s: levels must lie in 1 .. %d, got %d", who, MAX_LEVELS, d->levels);
  KFN_REQUIRE((d->H >> (d->levels - 1)) >= 2 && (d->W >> (d->levels - 1)) >= 2, "%s: %d levels leave the coarsest of %dx%d below 2x2", who,
              d->levels, d->H, d->W);
  KFN_REQUIRE(d->level >= 0 && d->level < d->levels, "%s: level %d outside 0 .. %d", who, d->level, d->levels - 1);
  KFN_REQUIRE(d->dfx > 0.0f && d->dfx <= FLT_MAX && d->dfy > 0.0f && d->dfy <= FLT_MAX && host_finite(d->du) && host_finite(d->dv),
              "%s: the focal lengths must be positive and the principal point finite", who);
  KFN_REQUIRE(d->near > 0.0f && d->near <= FLT_MAX, "%s: near must be positive and finite", who);
  return KFN_OK;
}

int checked_lattice(const kfn_track_desc* d, const char* who) {
  KFN_REQUIRE(d->nx > 1 && d->ny > 1 && d->nz > 1, "%s: the volume needs two lattice points an axis or more (%d x %d x %d)", who, d->nx,
              d->ny, d->nz);
  KFN_REQUIRE((long)d->nx * d->ny * d->nz < (1L << 31), "%s: %d x %d x %d lattice points: 2^31 or more", who, d->nx, d->ny, d->nz);
  KFN_REQUIRE(d->voxel > 0.0f && d->voxel <= FLT_MAX, "%s: voxel must be positive and finite", who);
  KFN_REQUIRE(d->trunc > 0.0f && d->trunc <= FLT_MAX, "%s: trunc must be positive and finite", who);
  KFN_REQUIRE(host_finite(d->ox) && host_finite(d->oy) && host_finite(d->oz), "%s: the origin must be finite", who);
  KFN_REQUIRE(d->far > d->near && d->far <= FLT_MAX, "%s: far must lie beyond near and be finite", who);
  KFN_REQUIRE(d->min_weight >= 1.0f && d->min_weight <= FLT_MAX, "%s: min_weight must be at least 1", who);
  return KFN_OK;
}

int icp_blocks(const Level& lv) { return (lv.H * lv.W + ICP_BLOCK - 1) / ICP_BLOCK; }

}  // namespace

extern "C" int kfn_track_scratch_bytes(const kfn_track_desc* d, size_t* bytes) {
  const int rc = checked_track(d, "kfn_track_scratch_bytes");
  if (rc != KFN_OK) return rc;
  KFN_REQUIRE(bytes, "kfn_track_scratch_bytes: null result");
  *bytes = (size_t)icp_blocks(level_of(d, 0)) * SUMS_LD * sizeof(double);
  return KFN_OK;
}

extern "C" int kfn_track_live_maps(const kfn_track_desc* d, const uint16_t* depth, float* live_v, float* live_n, void* stream) {
  const char* who = "kfn_track_live_maps";
  const int rc = checked_track(d, who);
  if (rc != KFN_OK) return rc;
  KFN_REQUIRE(depth && live_v && live_n, "%s: null buffer (depth, live_v and live_n are required)", who);
  KFN_REQUIRE(((uintptr_t)depth & 1) == 0 && ((uintptr_t)live_v & 15) == 0 && ((uintptr_t)live_n & 15) == 0,
              "%s: depth must be 2-byte aligned, the maps 16-byte", who);
  KFN_REQUIRE(d->scale > 0.0f && d->scale <= FLT_MAX, "%s: scale must be positive and finite", who);
  KFN_REQUIRE(d->raw_min >= 0 && d->raw_max <= 65535 && d->raw_min <= d->raw_max, "%s: bad validity window [%d, %d]", who, d->raw_min,
              d->raw_max);
  KFN_REQUIRE(d->pyr_dist >= 0.0f && d->pyr_dist <= FLT_MAX && d->jump >= 0.0f && d->jump <= FLT_MAX,
              "%s: pyr_dist and jump must be non-negative and finite", who);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float4* v = reinterpret_cast<float4*>(live_v);
  float4* n = reinterpret_cast<float4*>(live_n);
  Level prev = level_of(d, 0);
  hipLaunchKernelGGL(track_vertex0_kernel, dim3((unsigned)((prev.H * prev.W + TT - 1) / TT)), dim3(TT), 0, st, depth, v, prev, d->raw_min,
                     d->raw_max, d->scale);
  KFN_LAUNCH_CHECK("track_vertex0_kernel");
  for (int l = 1; l < d->levels; ++l) {
    const Level lv = level_of(d, l);
    hipLaunchKernelGGL(track_pyramid_kernel, dim3((unsigned)((lv.H * lv.W + TT - 1) / TT)), dim3(TT), 0, st, v + prev.off, v + lv.off, prev.W,
                       lv, d->pyr_dist);
    KFN_LAUNCH_CHECK("track_pyramid_kernel");
    prev = lv;
  }
  for (int l = 0; l < d->levels; ++l) {
    const Level lv = level_of(d, l);
    hipLaunchKernelGGL(track_normal_kernel, dim3((unsigned)((lv.H * lv.W + TT - 1) / TT)), dim3(TT), 0, st, v + lv.off, n + lv.off, lv.H, lv.W,
                       d->jump);
    KFN_LAUNCH_CHECK("track_normal_kernel");
  }
  return KFN_OK;
}

extern "C" int kfn_track_raycast(const kfn_track_desc* d, const float* tsdf, const kfn_track_state* state, float* model_v, float* model_n,
                                 void* stream) {
  const char* who = "kfn_track_raycast";
  int rc = checked_track(d, who);
  if (rc != KFN_OK) return rc;
  rc = checked_lattice(d, who);
  if (rc != KFN_OK) return rc;
  KFN_REQUIRE(tsdf && state && model_v && model_n, "%s: null buffer (tsdf, state, model_v and model_n are required)", who);
  KFN_REQUIRE(((uintptr_t)tsdf & 7) == 0 && ((uintptr_t)state & 7) == 0 && ((uintptr_t)model_v & 15) == 0 && ((uintptr_t)model_n & 15) == 0,
              "%s: tsdf and state must be 8-byte aligned, the maps 16-byte", who);
  RayArgs a;
  a.tsdf = reinterpret_cast<const float2*>(tsdf);
  a.state = state;
  a.mv = reinterpret_cast<float4*>(model_v);
  a.mn = reinterpret_cast<float4*>(model_n);
  a.lv = level_of(d, d->level);
  a.nx = d->nx; a.ny = d->ny; a.nz = d->nz;
  a.ox = d->ox; a.oy = d->oy; a.oz = d->oz; a.voxel = d->voxel; a.half_trunc = d->trunc * 0.5f;
  a.near = d->near; a.far = d->far; a.min_weight = d->min_weight;
  hipLaunchKernelGGL(track_raycast_kernel, dim3((unsigned)((a.lv.H * a.lv.W + TT - 1) / TT)), dim3(TT), 0, reinterpret_cast<hipStream_t>(stream), a);
  KFN_LAUNCH_CHECK("track_raycast_kernel");
  return KFN_OK;
}

extern "C" int kfn_track_icp_sums(const kfn_track_desc* d, const float* live_v, const float* live_n, const float* model_v,
                                  const float* model_n, const kfn_track_state* state, void* scratch, double* sums, void* stream) {
  const char* who = "kfn_track_icp_sums";
  const int rc = checked_track(d, who);
  if (rc != KFN_OK) return rc;
  KFN_REQUIRE(live_v && live_n && model_v && model_n && state && scratch && sums,
              "%s: null buffer (the four maps, state, scratch and sums are required)", who);
  KFN_REQUIRE((((uintptr_t)live_v | (uintptr_t)live_n | (uintptr_t)model_v | (uintptr_t)model_n) & 15) == 0 &&
                  (((uintptr_t)state | (uintptr_t)scratch | (uintptr_t)sums) & 7) == 0,
              "%s: the maps must be 16-byte aligned, state, scratch and sums 8-byte", who);
  KFN_REQUIRE(d->dist_max > 0.0f && d->dist_max <= FLT_MAX, "%s: dist_max must be positive and finite", who);
  KFN_REQUIRE(d->cos_min >= -1.0f && d->cos_min <= 1.0f, "%s: cos_min must lie in -1 .. 1", who);
  IcpArgs a;
  a.lv = reinterpret_cast<const float4*>(live_v);
  a.ln = reinterpret_cast<const float4*>(live_n);
  a.mv = reinterpret_cast<const float4*>(model_v);
  a.mn = reinterpret_cast<const float4*>(model_n);
  a.state = state;
  a.partial = static_cast<double*>(scratch);
  a.lvl = level_of(d, d->level);
  a.near = d->near; a.dist_max = d->dist_max; a.cos_min = d->cos_min;
  const int blocks = icp_blocks(a.lvl);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(track_icp_kernel, dim3((unsigned)blocks), dim3(TT), 0, st, a);
  KFN_LAUNCH_CHECK("track_icp_kernel");
  hipLaunchKernelGGL(track_reduce_kernel, dim3(1), dim3(64), 0, st, a.partial, blocks, sums);
  KFN_LAUNCH_CHECK("track_reduce_kernel");
  return KFN_OK;
}

extern "C" int kfn_track_update(const kfn_track_desc* d, const double* sums, kfn_track_state* state, void* stream) {
  const char* who = "kfn_track_update";
  const int rc = checked_track(d, who);
  if (rc != KFN_OK) return rc;
  KFN_REQUIRE(sums && state, "%s: null buffer (sums and state are required)", who);
  KFN_REQUIRE((((uintptr_t)sums | (uintptr_t)state) & 7) == 0, "%s: sums and state must be 8-byte aligned", who);
  KFN_REQUIRE(d->min_pairs >= 6, "%s: min_pairs must be at least 6, got %d", who, d->min_pairs);
  KFN_REQUIRE(d->pivot_floor >= 0.0f && d->pivot_floor < 1.0f, "%s: pivot_floor must lie in 0 .. 1", who);
  const Level lv = level_of(d, d->level);
  hipLaunchKernelGGL(track_update_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), sums, state, lv.H * lv.W, d->min_pairs,
                     (double)d->pivot_floor);
  KFN_LAUNCH_CHECK("track_update_kernel");
  return KFN_OK;
}

extern "C" int kfn_track_commit(const kfn_track_desc* d, kfn_track_state* state, float* pose_rows, double* trajectory, void* stream) {
  const char* who = "kfn_track_commit";
  const int rc = checked_track(d, who);
  if (rc != KFN_OK) return rc;
  KFN_REQUIRE(state && pose_rows && trajectory, "%s: null buffer (state, pose_rows and trajectory are required)", who);
  KFN_REQUIRE((((uintptr_t)state | (uintptr_t)trajectory) & 7) == 0 && ((uintptr_t)pose_rows & 3) == 0,
              "%s: state and trajectory must be 8-byte aligned, pose_rows 4-byte", who);
  KFN_REQUIRE(d->slot >= 0 && d->slot <= 65534, "%s: slot %d outside 0 .. 65534", who, d->slot);
  KFN_REQUIRE(d->traj_rows >= 1, "%s: traj_rows must be positive, got %d", who, d->traj_rows);
  KFN_REQUIRE(d->min_share >= 0.0f && d->min_share <= 1.0f, "%s: min_share must lie in 0 .. 1", who);
  KFN_REQUIRE(d->max_rms > 0.0f && d->max_step_m > 0.0f && d->max_step_rad > 0.0f, "%s: max_rms, max_step_m and max_step_rad must be positive",
              who);
  hipLaunchKernelGGL(track_commit_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), state, pose_rows + (long)d->slot * 12,
                     trajectory, d->traj_rows, (double)d->min_share, (double)d->max_rms, (double)d->max_step_m, (double)d->max_step_rad);
  KFN_LAUNCH_CHECK("track_commit_kernel");
  return KFN_OK;
}
