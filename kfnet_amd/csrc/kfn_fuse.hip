// kfn_fuse.hip -- depth maps fused into a truncated signed distance volume, and a triangle mesh extracted from it (gfx950).
// Compiled with -ffp-contract=off: every operation below is one rounded fp32 operation of DESIGN.md 6k, in that order, so a
// numpy float32 restatement (tests/fuse_ref.py) gives the same bits.  The quotients are IEEE divisions (hipcc's default
// for fp32), there is no transcendental and no floating-point atomic.
//
//   volume       lattice point (ix, iy, iz), x fastest; tsdf [nz][ny][nx] pairs (D, W), color [nz][ny][nx] quadruples
//                (r, g, b, wc); all zeros is the empty volume.  p = (ox + float(ix) voxel, oy + float(iy) voxel, oz + float(iz) voxel).
//   integrate    per voxel, frames b = 0 .. B-1 in this order:
//     1  P = poses[b][0..11]; a non-finite entry skips the frame.
//     2  dx = p.x - P[3], dy = p.y - P[7], dz = p.z - P[11];  X = (P[0] dx + P[4] dy) + P[8] dz;
//        Y = (P[1] dx + P[5] dy) + P[9] dz;  Z = (P[2] dx + P[6] dy) + P[10] dz           (kfn_render's transform)
//     3  Z < near or a non-finite coordinate: skip.
//     4  qx = X / Z, qy = Y / Z;  sx = qx dfx + du, sy = qy dfy + dv;  cf = rint(sx), rf = rint(sy) (ties to even);
//        skip unless 0 <= cf <= W-1 and 0 <= rf <= H-1, compared in float.
//     5  raw = depth[b][r][c]; outside [raw_min, raw_max]: skip.  dm = float(raw) scale.
//     6  s = dm - Z;  s < -trunc: skip.  f = min(s / trunc, 1).
//     7  D = (W D + f) / (W + 1);  W = min(W + 1, max_weight).
//     8  colour, when given and s <= trunc: cx = rint(qx fx + u), cy = rint(qy fy + v), inside the image as in 4:
//        ch = (wc ch + float(pixel)) / (wc + 1) per channel, then wc = min(wc + 1, max_weight).
//   extract      marching tetrahedra on the lattice.  A point is valid iff W >= min_weight, inside iff valid and D < 0.
//     edges      point v owns the edges to v + (1,0,0), (0,1,0), (0,0,1), (1,1,0), (1,0,1), (0,1,1), (1,1,1), in this order;
//                an edge carries a vertex iff its far end is in the grid, both ends are valid and exactly one is inside.
//                id = (vertices of all points with a lower linear index) + (rank among v's carrying edges).
//                a the owner end, b the far end: t = Da / (Da - Db), pos = pa + t (pb - pa) per component;
//                colour min(max(rint(ca + t (cb - ca)), 0), 255) when both ends have wc > 0, else 255.
//     cubes      the cube at v is cut into the tetrahedra {v, v + e_a, v + e_a + e_b, v + (1,1,1)} for (a, b, c) = xyz, xzy,
//                yxz, yzx, zxy, zyx; one is emitted iff its four corners are valid.  With m inside corners: 1 triangle for
//                m = 1 or 3, 2 for m = 2 (the quad split on a fixed diagonal), wound so that (v1 - v0) x (v2 - v0) points
//                from inside to outside.  index = (triangles of all cubes with a lower linear index) + (position in the
//                cube: tetrahedra 0..5, table order within one).
// The scan is plain launches -- block sums, a scan of the block sums, an add -- and no workgroup waits for another.
#include "kfn_common.h"
#include <cfloat>

namespace {

constexpr int FT = 256;                    // threads of a workgroup, every kernel here
constexpr int BX = 64, BY = 4;             // the brick of an integrate workgroup: a wave along x, four rows of y
constexpr int SCAN_ITEMS = 4;              // elements a thread of the scan takes
constexpr int SCAN_BLOCK = FT * SCAN_ITEMS;
constexpr int MAX_LEVELS = 8;

typedef unsigned long long u64;

struct FuseArgs {
  float2* tsdf;
  float4* color;
  const uint16_t* depth;
  const uint8_t* frames;
  const float* poses;
  int nx, ny, nz, B, H, W, raw_min, raw_max, bx, by;
  float ox, oy, oz, voxel, trunc, near, scale, max_weight, dfx, dfy, du, dv, fx, fy, u, v;
};

struct ExtractArgs {
  const float2* tsdf;
  const float4* color;
  uint32_t* vcnt;          // per point: vertex count, after the scan the first vertex id
  uint32_t* tcnt;          // per cube (indexed by its point): triangle count, after the scan the first triangle index
  uint8_t* mask;           // per point: which of its seven owned edges carry a vertex
  float* vertices;
  uint8_t* colors;
  int32_t* triangles;
  long n, cap_v, cap_t;
  int nx, ny, nz;
  float ox, oy, oz, voxel, min_weight;
};

__device__ __forceinline__ bool finite(float x) { return fabsf(x) <= FLT_MAX; }

// Thread = voxel (kx BX + lane, ky BY + row, iz) of brick blockIdx.x = (iz by + ky) bx + kx.  The voxel's (D, W) and colour
// stay in registers across the B frames; the pose and the intrinsics are wave-uniform (scalar registers).  A voxel that
// no frame touched is not stored: its bits are those it was loaded with.
__global__ __launch_bounds__(FT) void fuse_integrate_kernel(FuseArgs p) {
  const int lane = threadIdx.x & 63, row = threadIdx.x >> 6;
  unsigned brick = blockIdx.x;
  const int kx = (int)(brick % (unsigned)p.bx);
  brick /= (unsigned)p.bx;
  const int ky = (int)(brick % (unsigned)p.by);
  const int iz = (int)(brick / (unsigned)p.by);
  const int ix = kx * BX + lane, iy = ky * BY + row;
  if (ix >= p.nx || iy >= p.ny || iz >= p.nz) return;
  const long id = ((long)iz * p.ny + iy) * p.nx + ix;
  const float px = p.ox + (float)ix * p.voxel;
  const float py = p.oy + (float)iy * p.voxel;
  const float pz = p.oz + (float)iz * p.voxel;
  const float2 t0 = p.tsdf[id];
  float D = t0.x, Wt = t0.y;
  float4 col = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (p.color) col = p.color[id];
  bool touched = false, painted = false;
  const float wmax = (float)(p.W - 1), hmax = (float)(p.H - 1);
  const float ntrunc = -p.trunc;
  for (int b = 0; b < p.B; ++b) {
    float P[12];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      P[k] = p.poses[b * 12 + k];
      ok = ok && finite(P[k]);
    }
    if (!ok) continue;                      // b is uniform
    const float dx = px - P[3], dy = py - P[7], dz = pz - P[11];
    const float X = (P[0] * dx + P[4] * dy) + P[8] * dz;
    const float Y = (P[1] * dx + P[5] * dy) + P[9] * dz;
    const float Z = (P[2] * dx + P[6] * dy) + P[10] * dz;
    if (!(finite(X) && finite(Y) && finite(Z)) || Z < p.near) continue;
    const float qx = X / Z, qy = Y / Z;
    const float cf = rintf(qx * p.dfx + p.du), rf = rintf(qy * p.dfy + p.dv);
    if (!(cf >= 0.0f && cf <= wmax && rf >= 0.0f && rf <= hmax)) continue;
    const int raw = (int)p.depth[((long)b * p.H + (int)rf) * p.W + (int)cf];
    if (raw < p.raw_min || raw > p.raw_max) continue;
    const float dm = (float)raw * p.scale;
    const float s = dm - Z;
    if (s < ntrunc) continue;
    const float f = fminf(s / p.trunc, 1.0f);
    D = (Wt * D + f) / (Wt + 1.0f);
    Wt = fminf(Wt + 1.0f, p.max_weight);
    touched = true;
    if (p.color && s <= p.trunc) {
      const float xf = rintf(qx * p.fx + p.u), yf = rintf(qy * p.fy + p.v);
      if (xf >= 0.0f && xf <= wmax && yf >= 0.0f && yf <= hmax) {
        const uint8_t* px3 = p.frames + (((long)b * p.H + (int)yf) * p.W + (int)xf) * 3;
        const float w1 = col.w + 1.0f;
        col.x = (col.w * col.x + (float)px3[0]) / w1;
        col.y = (col.w * col.y + (float)px3[1]) / w1;
        col.z = (col.w * col.z + (float)px3[2]) / w1;
        col.w = fminf(w1, p.max_weight);
        painted = true;
      }
    }
  }
  if (touched) p.tsdf[id] = make_float2(D, Wt);
  if (painted) p.color[id] = col;
}

// ---- extraction -----------------------------------------------------------------------------------------------------------
// A corner of a cube is a 3-bit code (bit 0: +x, bit 1: +y, bit 2: +z).  EDGE_CODE: the far ends of the seven owned edges;
// EDGE_INDEX: its inverse.  TET: the corners of the six tetrahedra; the odd permutations (1, 2, 5) are mirror images, so
// their triangles are emitted with the last two vertices exchanged.
__constant__ unsigned char EDGE_CODE[7] = {1, 2, 4, 3, 5, 6, 7};
__constant__ unsigned char EDGE_INDEX[8] = {0, 0, 1, 3, 2, 4, 5, 6};
__constant__ unsigned char TET[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
__constant__ unsigned char TET_ODD[6] = {0, 1, 1, 0, 0, 1};
// For a tetrahedron of positive orientation (det [c1 - c0, c2 - c0, c3 - c0] > 0) and the mask m of its inside corners
// (bit j: corner j): TRI_COUNT[m] triangles, each three edges written 4 p + q (corners p < q).  One rule gives all of it:
// one inside corner i with the others j < k < l: the edges (i j), (i k), (i l) in the order whose normal points away from
// i; three inside: the same triangle of the outside corner, reversed; two inside i < j, outside k < l: the quad (i k), (i l),
// (j l), (j k) in the direction whose normals point from inside to outside, split into (q0 q1 q2) and (q0 q2 q3).
// tests/fuse_ref.py derives this table from the rule with determinants and compares.
__constant__ unsigned char TRI_COUNT[16] = {0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0};
__constant__ unsigned char TRI_EDGES[16][6] = {
    { 0,  0,  0,  0,  0,  0},   // 0000
    { 1,  2,  3,  0,  0,  0},   // 1000
    { 1,  7,  6,  0,  0,  0},   // 0100
    { 2,  3,  7,  2,  7,  6},   // 1100
    { 2,  6, 11,  0,  0,  0},   // 0010
    { 1,  6, 11,  1, 11,  3},   // 1010
    { 1,  7, 11,  1, 11,  2},   // 0110
    { 3,  7, 11,  0,  0,  0},   // 1110
    { 3, 11,  7,  0,  0,  0},   // 0001
    { 1,  2, 11,  1, 11,  7},   // 1001
    { 1,  3, 11,  1, 11,  6},   // 0101
    { 2, 11,  6,  0,  0,  0},   // 1101
    { 2,  6,  7,  2,  7,  3},   // 0011
    { 1,  6,  7,  0,  0,  0},   // 1011
    { 1,  3,  2,  0,  0,  0},   // 0111
    { 0,  0,  0,  0,  0,  0},   // 1111
};

struct Corners {
  unsigned valid, inside;        // bit c: the corner with code c (0 where it lies outside the grid)
  bool cube;
};

__device__ __forceinline__ long corner_offset(const ExtractArgs& p, int code) {
  return (long)(code & 1) + (long)((code >> 1) & 1) * p.nx + (long)((code >> 2) & 1) * p.nx * p.ny;
}

__device__ __forceinline__ Corners corners_of(const ExtractArgs& p, long i, int ix, int iy, int iz) {
  Corners c;
  c.valid = c.inside = 0;
  const bool mx = ix + 1 < p.nx, my = iy + 1 < p.ny, mz = iz + 1 < p.nz;
  c.cube = mx && my && mz;
#pragma unroll
  for (int code = 0; code < 8; ++code) {
    const bool in_grid = (!(code & 1) || mx) && (!(code & 2) || my) && (!(code & 4) || mz);
    if (in_grid) {
      const float2 t = p.tsdf[i + corner_offset(p, code)];
      const bool valid = t.y >= p.min_weight;
      if (valid) c.valid |= 1u << code;
      if (valid && t.x < 0.0f) c.inside |= 1u << code;
    }
  }
  return c;
}

__device__ __forceinline__ unsigned edge_mask(const Corners& c) {
  unsigned m = 0;
  if (c.valid & 1u) {
#pragma unroll
    for (int e = 0; e < 7; ++e) {
      const int code = EDGE_CODE[e];
      if (((c.valid >> code) & 1u) && (((c.inside >> code) ^ c.inside) & 1u)) m |= 1u << e;
    }
  }
  return m;
}

__global__ __launch_bounds__(FT) void fuse_count_kernel(ExtractArgs p) {
  const long i = (long)blockIdx.x * FT + threadIdx.x;
  if (i >= p.n) return;
  const int ix = (int)(i % p.nx), iy = (int)((i / p.nx) % p.ny), iz = (int)(i / ((long)p.nx * p.ny));
  const Corners c = corners_of(p, i, ix, iy, iz);
  const unsigned m = edge_mask(c);
  unsigned tris = 0;
  if (c.cube) {
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      unsigned all = 1, in = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        all &= (c.valid >> TET[k][j]) & 1u;
        in |= ((c.inside >> TET[k][j]) & 1u) << j;
      }
      if (all) tris += TRI_COUNT[in];
    }
  }
  p.mask[i] = (uint8_t)m;
  p.vcnt[i] = (unsigned)__popc(m);
  p.tcnt[i] = tris;
}

__device__ __forceinline__ float channel(float v) { return fminf(fmaxf(rintf(v), 0.0f), 255.0f); }

__global__ __launch_bounds__(FT) void fuse_emit_kernel(ExtractArgs p) {
  const long i = (long)blockIdx.x * FT + threadIdx.x;
  if (i >= p.n) return;
  const int ix = (int)(i % p.nx), iy = (int)((i / p.nx) % p.ny), iz = (int)(i / ((long)p.nx * p.ny));
  const unsigned m = p.mask[i];
  if (m) {
    const float2 ta = p.tsdf[i];
    const float ax = p.ox + (float)ix * p.voxel, ay = p.oy + (float)iy * p.voxel, az = p.oz + (float)iz * p.voxel;
    float4 ca = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (p.color) ca = p.color[i];
    long id = (long)p.vcnt[i];
    for (int e = 0; e < 7; ++e) {
      if (!((m >> e) & 1u)) continue;
      const int code = EDGE_CODE[e];
      if (id < p.cap_v) {
        const long j = i + corner_offset(p, code);
        const float2 tb = p.tsdf[j];
        const float t = ta.x / (ta.x - tb.x);
        const float bx = p.ox + (float)(ix + (code & 1)) * p.voxel;
        const float by = p.oy + (float)(iy + ((code >> 1) & 1)) * p.voxel;
        const float bz = p.oz + (float)(iz + ((code >> 2) & 1)) * p.voxel;
        float* dst = p.vertices + id * 3;
        dst[0] = ax + t * (bx - ax);
        dst[1] = ay + t * (by - ay);
        dst[2] = az + t * (bz - az);
        if (p.colors) {
          float r = 255.0f, g = 255.0f, bl = 255.0f;
          if (p.color) {
            const float4 cb = p.color[j];
            if (ca.w > 0.0f && cb.w > 0.0f) {
              r = channel(ca.x + t * (cb.x - ca.x));
              g = channel(ca.y + t * (cb.y - ca.y));
              bl = channel(ca.z + t * (cb.z - ca.z));
            }
          }
          uint8_t* cd = p.colors + id * 3;
          cd[0] = (uint8_t)r; cd[1] = (uint8_t)g; cd[2] = (uint8_t)bl;
        }
      }
      ++id;
    }
  }
  if (!(ix + 1 < p.nx && iy + 1 < p.ny && iz + 1 < p.nz)) return;
  long tri = (long)p.tcnt[i];
  // a cube with no triangle is the common case: the next point's first index tells without the eight loads (a cube's
  // point is never the last of the volume)
  if (i + 1 < p.n && (long)p.tcnt[i + 1] == tri) return;
  const Corners c = corners_of(p, i, ix, iy, iz);
  for (int k = 0; k < 6; ++k) {
    unsigned all = 1, in = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      all &= (c.valid >> TET[k][j]) & 1u;
      in |= ((c.inside >> TET[k][j]) & 1u) << j;
    }
    if (!all) continue;
    const int count = TRI_COUNT[in];
    for (int j = 0; j < count; ++j, ++tri) {
      if (tri >= p.cap_t) continue;
      int ids[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const int pq = TRI_EDGES[in][j * 3 + q];
        const int ca = TET[k][pq >> 2], cb = TET[k][pq & 3];
        const long owner = i + corner_offset(p, ca);
        const int e = EDGE_INDEX[ca ^ cb];
        ids[q] = (int)(p.vcnt[owner] + (unsigned)__popc((unsigned)p.mask[owner] & ((1u << e) - 1u)));
      }
      int32_t* dst = p.triangles + tri * 3;
      const bool odd = TET_ODD[k] != 0;
      dst[0] = ids[0];
      dst[1] = odd ? ids[2] : ids[1];
      dst[2] = odd ? ids[1] : ids[2];
    }
  }
}

// ---- the scan: block sums, a scan of the block sums, an add ------------------------------------------------------------------
// blockIdx.y picks the array (vertex counts, triangle counts).  Each workgroup replaces its SCAN_BLOCK elements by their
// exclusive prefix sums within the block and writes the block's total; nothing waits for another workgroup.
template <typename T>
__global__ __launch_bounds__(FT) void fuse_scan_kernel(T* data0, T* data1, long n, u64* sums0, u64* sums1) {
  __shared__ u64 buf[FT];
  T* data = blockIdx.y ? data1 : data0;
  u64* sums = blockIdx.y ? sums1 : sums0;
  const int tid = threadIdx.x;
  const long base = (long)blockIdx.x * SCAN_BLOCK + (long)tid * SCAN_ITEMS;
  T v[SCAN_ITEMS];
  u64 s = 0;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) {
    v[k] = base + k < n ? data[base + k] : (T)0;
    s += (u64)v[k];
  }
  buf[tid] = s;
  __syncthreads();
  for (int off = 1; off < FT; off <<= 1) {
    const u64 add = tid >= off ? buf[tid - off] : 0;
    __syncthreads();
    buf[tid] += add;
    __syncthreads();
  }
  u64 run = buf[tid] - s;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) {
    if (base + k < n) data[base + k] = (T)run;
    run += (u64)v[k];
  }
  if (tid == FT - 1) sums[blockIdx.x] = buf[FT - 1];
}

template <typename T>
__global__ __launch_bounds__(FT) void fuse_scan_add_kernel(T* data0, T* data1, long n, const u64* sums0, const u64* sums1) {
  T* data = blockIdx.y ? data1 : data0;
  const u64* sums = blockIdx.y ? sums1 : sums0;
  const long i = (long)blockIdx.x * FT + threadIdx.x;
  if (i < n) data[i] += (T)sums[i / SCAN_BLOCK];
}

// the sizes of the scan's levels: sz[0] = n, sz[k + 1] = ceil(sz[k] / SCAN_BLOCK), down to sz[L] = 1
int scan_levels(long n, long* sz) {
  int L = 0;
  sz[0] = n;
  do {
    sz[L + 1] = (sz[L] + SCAN_BLOCK - 1) / SCAN_BLOCK;
    ++L;
  } while (sz[L] > 1 && L + 1 < MAX_LEVELS);
  return L;
}

long level_words(long n) {        // u64 words one array's levels 1 .. L-1 take
  long sz[MAX_LEVELS + 1];
  const int L = scan_levels(n, sz);
  long words = 0;
  for (int k = 1; k < L; ++k) words += sz[k];
  return words;
}

bool host_finite(float x) { return x - x == 0.0f; }

int checked_volume(const kfn_fuse_desc* d, const char* who) {
  KFN_REQUIRE(d, "%s: null descriptor", who);
  KFN_REQUIRE(d->struct_size == (int32_t)sizeof(kfn_fuse_desc), "%s: struct_size %d, expected %d", who, (int)d->struct_size,
              (int)sizeof(kfn_fuse_desc));
  KFN_REQUIRE(d->nx > 0 && d->ny > 0 && d->nz > 0, "%s: the volume's dimensions must be positive (%d x %d x %d)", who, d->nx, d->ny,
              d->nz);
  KFN_REQUIRE((long)d->nx * d->ny * d->nz < (1L << 31), "%s: %d x %d x %d lattice points: 2^31 or more", who, d->nx, d->ny, d->nz);
  KFN_REQUIRE(d->voxel > 0.0f && d->voxel <= FLT_MAX, "%s: voxel must be positive and finite", who);
  KFN_REQUIRE(host_finite(d->ox) && host_finite(d->oy) && host_finite(d->oz), "%s: the origin must be finite", who);
  return KFN_OK;
}

int checked_extract(const kfn_fuse_desc* d, const char* who) {
  const int rc = checked_volume(d, who);
  if (rc != KFN_OK) return rc;
  KFN_REQUIRE(d->min_weight >= 1.0f && d->min_weight <= FLT_MAX, "%s: min_weight must be at least 1", who);
  return KFN_OK;
}

void extract_args(const kfn_fuse_desc* d, const float* tsdf, const float* color, void* scratch, ExtractArgs* a) {
  const long n = (long)d->nx * d->ny * d->nz;
  a->tsdf = reinterpret_cast<const float2*>(tsdf);
  a->color = reinterpret_cast<const float4*>(color);
  a->vcnt = static_cast<uint32_t*>(scratch);
  a->tcnt = a->vcnt + n;
  a->mask = reinterpret_cast<uint8_t*>(reinterpret_cast<u64*>(a->tcnt + n) + 2 * level_words(n));
  a->vertices = nullptr; a->colors = nullptr; a->triangles = nullptr;
  a->n = n; a->cap_v = 0; a->cap_t = 0;
  a->nx = d->nx; a->ny = d->ny; a->nz = d->nz;
  a->ox = d->ox; a->oy = d->oy; a->oz = d->oz; a->voxel = d->voxel; a->min_weight = d->min_weight;
}

}  // namespace

extern "C" int kfn_fuse_scratch_bytes(const kfn_fuse_desc* d, size_t* bytes) {
  const int rc = checked_volume(d, "kfn_fuse_scratch_bytes");
  if (rc != KFN_OK) return rc;
  KFN_REQUIRE(bytes, "kfn_fuse_scratch_bytes: null result");
  const size_t n = (size_t)d->nx * d->ny * d->nz;
  // two uint32 arrays, both arrays' upper levels as 64-bit words, one byte of edge mask a point
  *bytes = 8 * n + 16 * (size_t)level_words((long)n) + ((n + 7) & ~(size_t)7);
  return KFN_OK;
}

extern "C" int kfn_fuse_integrate(const kfn_fuse_desc* d, float* tsdf, float* color, const uint16_t* depth, const uint8_t* frames,
                                  const float* poses, void* stream) {
  const char* who = "kfn_fuse_integrate";
  const int rc = checked_volume(d, who);
  if (rc != KFN_OK) return rc;
  KFN_REQUIRE(tsdf && depth && poses, "%s: null buffer (tsdf, depth and poses are required)", who);
  KFN_REQUIRE((frames == nullptr) == (color == nullptr), "%s: frames and color go together: both NULL or both given", who);
  KFN_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0, "%s: sizes must be positive (B %d, %dx%d)", who, d->B, d->H, d->W);
  KFN_REQUIRE(d->B <= 65535, "%s: %d frames: at most 65535 in one call", who, d->B);
  KFN_REQUIRE(d->trunc > 0.0f && d->trunc <= FLT_MAX, "%s: trunc must be positive and finite", who);
  KFN_REQUIRE(d->near > 0.0f && d->near <= FLT_MAX, "%s: near must be positive and finite", who);
  KFN_REQUIRE(d->scale > 0.0f && d->scale <= FLT_MAX, "%s: scale must be positive and finite", who);
  KFN_REQUIRE(d->max_weight >= 1.0f && d->max_weight <= FLT_MAX, "%s: max_weight must be at least 1", who);
  KFN_REQUIRE(d->raw_min >= 0 && d->raw_max <= 65535 && d->raw_min <= d->raw_max, "%s: bad validity window [%d, %d]", who,
              d->raw_min, d->raw_max);
  KFN_REQUIRE(((uintptr_t)tsdf & 7) == 0 && ((uintptr_t)color & 15) == 0 && ((uintptr_t)depth & 1) == 0 && ((uintptr_t)poses & 3) == 0,
              "%s: tsdf must be 8-byte aligned, color 16-byte, depth 2-byte, poses 4-byte", who);
  FuseArgs a;
  a.tsdf = reinterpret_cast<float2*>(tsdf); a.color = reinterpret_cast<float4*>(color);
  a.depth = depth; a.frames = frames; a.poses = poses;
  a.nx = d->nx; a.ny = d->ny; a.nz = d->nz; a.B = d->B; a.H = d->H; a.W = d->W; a.raw_min = d->raw_min; a.raw_max = d->raw_max;
  a.bx = (d->nx + BX - 1) / BX; a.by = (d->ny + BY - 1) / BY;
  a.ox = d->ox; a.oy = d->oy; a.oz = d->oz; a.voxel = d->voxel; a.trunc = d->trunc; a.near = d->near; a.scale = d->scale;
  a.max_weight = d->max_weight; a.dfx = d->dfx; a.dfy = d->dfy; a.du = d->du; a.dv = d->dv;
  a.fx = d->fx; a.fy = d->fy; a.u = d->u; a.v = d->v;
  const long bricks = (long)a.bx * a.by * a.nz;           // < 2^31: there are fewer bricks than lattice points
  hipLaunchKernelGGL(fuse_integrate_kernel, dim3((unsigned)bricks), dim3(FT), 0, reinterpret_cast<hipStream_t>(stream), a);
  KFN_LAUNCH_CHECK("fuse_integrate_kernel");
  return KFN_OK;
}

extern "C" int kfn_fuse_extract_count(const kfn_fuse_desc* d, const float* tsdf, void* scratch, uint64_t* totals, void* stream) {
  const char* who = "kfn_fuse_extract_count";
  const int rc = checked_extract(d, who);
  if (rc != KFN_OK) return rc;
  KFN_REQUIRE(tsdf && scratch && totals, "%s: null buffer (tsdf, scratch and totals are required)", who);
  KFN_REQUIRE(((uintptr_t)tsdf & 7) == 0 && ((uintptr_t)scratch & 7) == 0 && ((uintptr_t)totals & 7) == 0,
              "%s: tsdf, scratch and totals must be 8-byte aligned", who);
  ExtractArgs a;
  extract_args(d, tsdf, nullptr, scratch, &a);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(fuse_count_kernel, dim3((unsigned)((a.n + FT - 1) / FT)), dim3(FT), 0, st, a);
  KFN_LAUNCH_CHECK("fuse_count_kernel");
  long sz[MAX_LEVELS + 1];
  const int L = scan_levels(a.n, sz);
  KFN_REQUIRE(sz[L] == 1, "%s: the scan needs more levels than it has", who);
  // level k >= 1 of array j: 64-bit words behind the two uint32 arrays; level L is the total
  u64* words = reinterpret_cast<u64*>(a.tcnt + a.n);
  const long per_array = level_words(a.n);
  u64* level[2][MAX_LEVELS + 1];
  for (int j = 0; j < 2; ++j) {
    long off = 0;
    for (int k = 1; k < L; ++k) {
      level[j][k] = words + j * per_array + off;
      off += sz[k];
    }
    level[j][L] = reinterpret_cast<u64*>(totals) + j;
  }
  hipLaunchKernelGGL(fuse_scan_kernel<uint32_t>, dim3((unsigned)sz[1], 2), dim3(FT), 0, st, a.vcnt, a.tcnt, sz[0], level[0][1], level[1][1]);
  KFN_LAUNCH_CHECK("fuse_scan_kernel");
  for (int k = 1; k < L; ++k) {
    hipLaunchKernelGGL(fuse_scan_kernel<u64>, dim3((unsigned)sz[k + 1], 2), dim3(FT), 0, st, level[0][k], level[1][k], sz[k],
                       level[0][k + 1], level[1][k + 1]);
    KFN_LAUNCH_CHECK("fuse_scan_kernel");
  }
  for (int k = L - 2; k >= 1; --k) {
    hipLaunchKernelGGL(fuse_scan_add_kernel<u64>, dim3((unsigned)((sz[k] + FT - 1) / FT), 2), dim3(FT), 0, st, level[0][k], level[1][k],
                       sz[k], level[0][k + 1], level[1][k + 1]);
    KFN_LAUNCH_CHECK("fuse_scan_add_kernel");
  }
  if (L >= 2) {
    hipLaunchKernelGGL(fuse_scan_add_kernel<uint32_t>, dim3((unsigned)((sz[0] + FT - 1) / FT), 2), dim3(FT), 0, st, a.vcnt, a.tcnt, sz[0],
                       level[0][1], level[1][1]);
    KFN_LAUNCH_CHECK("fuse_scan_add_kernel");
  }
  return KFN_OK;
}

extern "C" int kfn_fuse_extract(const kfn_fuse_desc* d, const float* tsdf, const float* color, const void* scratch, float* vertices,
                                uint8_t* colors, int32_t* triangles, int64_t cap_vertices, int64_t cap_triangles, void* stream) {
  const char* who = "kfn_fuse_extract";
  const int rc = checked_extract(d, who);
  if (rc != KFN_OK) return rc;
  KFN_REQUIRE(tsdf && scratch && vertices && triangles, "%s: null buffer (tsdf, scratch, vertices and triangles are required)", who);
  KFN_REQUIRE(cap_vertices >= 0 && cap_triangles >= 0 && cap_vertices < (1LL << 31) && cap_triangles < (1LL << 31),
              "%s: capacities must lie in 0 .. 2^31 - 1 (%lld vertices, %lld triangles)", who, (long long)cap_vertices,
              (long long)cap_triangles);
  KFN_REQUIRE(((uintptr_t)tsdf & 7) == 0 && ((uintptr_t)color & 15) == 0 && ((uintptr_t)scratch & 7) == 0 &&
                  ((uintptr_t)vertices & 3) == 0 && ((uintptr_t)triangles & 3) == 0,
              "%s: tsdf and scratch must be 8-byte aligned, color 16-byte, vertices and triangles 4-byte", who);
  ExtractArgs a;
  extract_args(d, tsdf, color, const_cast<void*>(scratch), &a);
  a.vertices = vertices; a.colors = colors; a.triangles = triangles;
  a.cap_v = (long)cap_vertices; a.cap_t = (long)cap_triangles;
  hipLaunchKernelGGL(fuse_emit_kernel, dim3((unsigned)((a.n + FT - 1) / FT)), dim3(FT), 0, reinterpret_cast<hipStream_t>(stream), a);
  KFN_LAUNCH_CHECK("fuse_emit_kernel");
  return KFN_OK;
}
