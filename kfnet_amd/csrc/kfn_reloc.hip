// kfn_reloc.hip -- a lost tracker relocalised from fern-coded keyframes (gfx950): every frame is coded by a few hundred binary
// tests on the coarsest live vertex map (and the staged frame), the tracked frames whose code differs enough from those kept
// become keyframes with their pose, and after a loss ICP restarts from the poses of the nearest codes (include/kfnet_hip.h,
// the kfn_reloc_* block; tests/reloc_ref.py restates it in numpy).  Compiled with -ffp-contract=off like kfn_track.hip.  The
// arithmetic is integer, or copies of fp64 poses; the only floating-point comparisons are z > threshold and the two gates.
// Every launch decides what to do from the records on the device; every index taken from a record is compared against its
// bound before it is used.  No floating-point atomics, no workgroup waits for another: two launches give the same bits.
#include "kfn_common.h"
#include <climits>

namespace {

constexpr int TT = 256;                    // threads of a workgroup of the encode, distance and select kernels
constexpr int WAVES = TT / 64;
constexpr int MAX_LEVELS = 4;
constexpr int MAX_FERNS = 4096, MAX_CAPACITY = 65536, MAX_TRIES = 4;
constexpr int TRAJ_LD = 20;                // doubles a trajectory row takes (kfn_track.hip)
constexpr int ROW_LD = 8;                  // int32 a row of reloc_rows takes
constexpr int INDEX_BITS = 16;             // a key is d 2^16 + index: d <= 4096, index < 65536

struct EncodeArgs {
  const int32_t* table;
  const float4* live_v;
  const uint8_t* frame;
  uint8_t* code;
  int ferns, Hl, Wl, W, level;
  long off;
};

// One thread per fern.  The position is tested before any use; a fern outside the level codes 0 and reads nothing.
__global__ __launch_bounds__(TT) void reloc_encode_kernel(EncodeArgs p) {
  const int f = blockIdx.x * TT + threadIdx.x;
  if (f >= p.ferns) return;
  const int x = p.table[4 * f], y = p.table[4 * f + 1];
  int byte = 0;
  if (x >= 0 && x < p.Wl && y >= 0 && y < p.Hl) {
    const float4 v = p.live_v[p.off + (long)y * p.Wl + x];
    const float thr = __int_as_float(p.table[4 * f + 2]);
    if (v.w != 0.0f && v.z > thr) byte = 1;
    if (p.frame) {
      const int side = 1 << p.level, area = side * side;
      const int packed = p.table[4 * f + 3];
      int sum[3] = {0, 0, 0};
      for (int dy = 0; dy < side; ++dy) {
        const uint8_t* row = p.frame + ((long)(y * side + dy) * p.W + (long)x * side) * 3;
        for (int dx = 0; dx < side; ++dx) {
          sum[0] += (int)row[3 * dx];
          sum[1] += (int)row[3 * dx + 1];
          sum[2] += (int)row[3 * dx + 2];
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (sum[c] > ((packed >> (8 * c)) & 255) * area) byte |= 2 << c;
      }
    }
  }
  p.code[f] = (uint8_t)byte;
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ int wave_min_i32(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
  return v;
}

__device__ __forceinline__ int clamped(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One wave per keyframe slot; slots >= n (n clamped to capacity) exit.
__global__ __launch_bounds__(TT) void reloc_distance_kernel(const uint8_t* code, const uint8_t* codes, const kfn_reloc_state* rs,
                                                            int32_t* dist, int ferns, int capacity) {
  const int slot = blockIdx.x * WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int n = clamped(rs->n, 0, capacity);
  if (slot >= n) return;
  const uint8_t* key = codes + (long)slot * ferns;
  int d = 0;
  for (int f = lane; f < ferns; f += 64) d += code[f] != key[f] ? 1 : 0;
  d = wave_sum_i32(d);
  if (lane == 0) dist[slot] = d;
}

// One workgroup: the `tries` least keys d 2^16 + index in ascending order, one round a key; the keys are distinct.
__global__ __launch_bounds__(TT) void reloc_select_kernel(const int32_t* dist, kfn_reloc_state* rs, int ferns, int capacity, int tries) {
  __shared__ int part[WAVES];
  const int tid = threadIdx.x;
  const int n = clamped(rs->n, 0, capacity);
  int prev = -1;
  for (int r = 0; r < MAX_TRIES; ++r) {
    int best = INT_MAX;
    if (r < tries) {
      for (int s = tid; s < n; s += TT) {
        const int key = (clamped(dist[s], 0, ferns) << INDEX_BITS) | s;
        if (key > prev && key < best) best = key;
      }
    }
    best = wave_min_i32(best);
    if ((tid & 63) == 0) part[tid >> 6] = best;
    __syncthreads();
    best = min(min(part[0], part[1]), min(part[2], part[3]));
    __syncthreads();
    if (tid == 0) {
      const bool found = best != INT_MAX;
      rs->cand_d[r] = found ? best >> INDEX_BITS : ferns + 1;
      rs->cand_index[r] = found ? best & ((1 << INDEX_BITS) - 1) : -1;
      if (r == 0) rs->min_d = found ? best >> INDEX_BITS : ferns + 1;
    }
    prev = best;                           // INT_MAX once the keys run out: no later round finds one
  }
  if (tid == 0) rs->candidates = n < tries ? n : tries;
}

__global__ __launch_bounds__(64) void reloc_seed_kernel(kfn_reloc_state* rs, kfn_track_state* ts, const double* key_poses, int capacity,
                                                        int tries) {
  if (threadIdx.x != 0) return;
  const int n = clamped(rs->n, 0, capacity);
  const int candidates = clamped(rs->candidates, 0, n < tries ? n : tries);
  const int streak = rs->streak;
  if (streak <= 0 || candidates <= 0) return;
  const int index = rs->cand_index[(streak - 1) % candidates];
  if (index < 0 || index >= n) return;
  const double* pose = key_poses + (long)index * 12;
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    const double v = pose[k];
    ts->committed[k] = v;
    ts->estimate[k] = v;
  }
  rs->seeded = 1;
  rs->seed_key = index;
}

struct SettleArgs {
  kfn_reloc_state* rs;
  kfn_track_state* ts;
  const uint8_t* code;
  uint8_t* codes;
  double* key_poses;
  float* pose_row;
  double* trajectory;
  int32_t* rows;
  int ferns, capacity, tries, harvest, n_rows, traj_rows, first;
  double min_share, max_rms;
};

// One wave.  Every lane reads the records and takes the same decisions; the lanes share the copy of the code, lane 0 writes.
__global__ __launch_bounds__(64) void reloc_settle_kernel(SettleArgs p) {
  const int lane = threadIdx.x;
  kfn_reloc_state* rs = p.rs;
  kfn_track_state* ts = p.ts;
  int n = clamped(rs->n, 0, p.capacity);
  int streak = rs->streak < 0 ? 0 : rs->streak;
  const int candidates = clamped(rs->candidates, 0, n < p.tries ? n : p.tries);
  const int min_d = rs->min_d, nearest = candidates > 0 ? rs->cand_index[0] : -1;
  const bool seeded = !p.first && rs->seeded == 1;
  const int seed_key = rs->seed_key;
  const int row = ts->frame - 1;
  bool tracked = p.first != 0;
  if (!p.first && row >= 0 && row < p.traj_rows) tracked = p.trajectory[(long)row * TRAJ_LD + 12] == 0.0;
  const double share = ts->last_share, rms = ts->last_rms;
  __syncthreads();
  int added = -1, demoted = 0;
  if (tracked && seeded && !(share >= p.min_share && rms <= p.max_rms)) {
    demoted = 1;
    tracked = false;
  }
  if (tracked && !seeded && (n == 0 || min_d > p.harvest) && n < p.capacity) {
    added = n;
    uint8_t* key = p.codes + (long)n * p.ferns;
    for (int f = lane; f < p.ferns; f += 64) key[f] = p.code[f];
  }
  if (lane != 0) return;
  const double nan = __builtin_nan("");
  if (tracked) {
    streak = 0;
    if (seeded) rs->recovered = rs->recovered + 1;
    if (added >= 0) {
#pragma unroll
      for (int k = 0; k < 12; ++k) p.key_poses[(long)added * 12 + k] = ts->committed[k];
      n = n + 1;
    }
  } else {
    if (demoted) {
#pragma unroll
      for (int k = 0; k < 12; ++k) p.pose_row[k] = __builtin_nanf("");
      if (row >= 0 && row < p.traj_rows) {
        double* t = p.trajectory + (long)row * TRAJ_LD;
#pragma unroll
        for (int k = 0; k < 12; ++k) t[k] = nan;
        t[12] = 1.0;
      }
      ts->lost = ts->lost + 1;
    }
    if (streak == 0 && !seeded) {          // a streak begins: the committed pose is the last one truly tracked
#pragma unroll
      for (int k = 0; k < 12; ++k) rs->anchor[k] = ts->committed[k];
    }
    if (streak < INT_MAX) streak = streak + 1;
    if (seeded) {
#pragma unroll
      for (int k = 0; k < 12; ++k) {
        const double v = rs->anchor[k];
        ts->committed[k] = v;
        ts->estimate[k] = v;
      }
    }
  }
  rs->n = n;
  rs->streak = streak;
  rs->seeded = 0;
  if (row >= 0 && row < p.n_rows) {
    int32_t* r = p.rows + (long)row * ROW_LD;
    r[0] = min_d;
    r[1] = nearest;
    r[2] = seeded ? seed_key : -1;
    r[3] = added;
    r[4] = streak;
    r[5] = candidates;
    r[6] = demoted;
    r[7] = 0;
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
int checked_reloc(const kfn_reloc_desc* d, const char* who) {
  KFN_REQUIRE(d, "%s: null descriptor", who);
  KFN_REQUIRE(d->struct_size == (int32_t)sizeof(kfn_reloc_desc), "%s: struct_size %d, expected %d", who, (int)d->struct_size,
              (int)sizeof(kfn_reloc_desc));
  KFN_REQUIRE(d->H > 0 && d->W > 0 && (long)d->H * d->W < (1L << 28), "%s: the image size must be positive and below 2^28 pixels (%dx%d)",
              who, d->H, d->W);
  KFN_REQUIRE(d->levels >= 1 && d->levels <= MAX_LEVELS, "%s: levels must lie in 1 .. %d, got %d", who, MAX_LEVELS, d->levels);
  KFN_REQUIRE((d->H >> (d->levels - 1)) >= 2 && (d->W >> (d->levels - 1)) >= 2, "%s: %d levels leave the coarsest of %dx%d below 2x2", who,
              d->levels, d->H, d->W);
  KFN_REQUIRE(d->reloc_level >= 0 && d->reloc_level < d->levels, "%s: reloc_level %d outside 0 .. %d", who, d->reloc_level, d->levels - 1);
  KFN_REQUIRE(d->ferns >= 1 && d->ferns <= MAX_FERNS, "%s: ferns must lie in 1 .. %d, got %d", who, MAX_FERNS, d->ferns);
  KFN_REQUIRE(d->capacity >= 1 && d->capacity <= MAX_CAPACITY, "%s: capacity must lie in 1 .. %d, got %d", who, MAX_CAPACITY, d->capacity);
  KFN_REQUIRE(d->tries >= 1 && d->tries <= MAX_TRIES, "%s: tries must lie in 1 .. %d, got %d", who, MAX_TRIES, d->tries);
  KFN_REQUIRE(d->rows >= 1, "%s: rows must be positive, got %d", who, d->rows);
  KFN_REQUIRE(d->harvest >= 0 && d->harvest <= d->ferns, "%s: harvest %d outside 0 .. ferns = %d", who, d->harvest, d->ferns);
  KFN_REQUIRE(d->colour == 0 || d->colour == 1, "%s: colour must be 0 or 1, got %d", who, d->colour);
  return KFN_OK;
}

}  // namespace

extern "C" int kfn_reloc_encode(const kfn_reloc_desc* d, const int32_t* table, const float* live_v, const uint8_t* frame, uint8_t* code,
                                void* stream) {
  const char* who = "kfn_reloc_encode";
  const int rc = checked_reloc(d, who);
  if (rc != KFN_OK) return rc;
  KFN_REQUIRE(table && live_v && code, "%s: null buffer (table, live_v and code are required)", who);
  KFN_REQUIRE(((uintptr_t)table & 15) == 0 && ((uintptr_t)live_v & 15) == 0, "%s: table and live_v must be 16-byte aligned", who);
  KFN_REQUIRE((d->colour != 0) == (frame != nullptr), "%s: a colour table goes with a frame: give both or neither", who);
  EncodeArgs a;
  a.table = table;
  a.live_v = reinterpret_cast<const float4*>(live_v);
  a.frame = frame;
  a.code = code;
  a.ferns = d->ferns;
  a.W = d->W;
  a.level = d->reloc_level;
  a.Hl = d->H; a.Wl = d->W; a.off = 0;
  for (int k = 0; k < d->reloc_level; ++k) {
    a.off += (long)a.Hl * a.Wl;
    a.Hl /= 2; a.Wl /= 2;
  }
  hipLaunchKernelGGL(reloc_encode_kernel, dim3((unsigned)((d->ferns + TT - 1) / TT)), dim3(TT), 0, reinterpret_cast<hipStream_t>(stream), a);
  KFN_LAUNCH_CHECK("reloc_encode_kernel");
  return KFN_OK;
}

extern "C" int kfn_reloc_search(const kfn_reloc_desc* d, const uint8_t* code, const uint8_t* codes, kfn_reloc_state* state, int32_t* dist,
                                void* stream) {
  const char* who = "kfn_reloc_search";
  const int rc = checked_reloc(d, who);
  if (rc != KFN_OK) return rc;
  KFN_REQUIRE(code && codes && state && dist, "%s: null buffer (code, codes, state and dist are required)", who);
  KFN_REQUIRE(((uintptr_t)state & 7) == 0 && ((uintptr_t)dist & 3) == 0, "%s: state must be 8-byte aligned, dist 4-byte", who);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(reloc_distance_kernel, dim3((unsigned)((d->capacity + WAVES - 1) / WAVES)), dim3(TT), 0, st, code, codes, state, dist,
                     d->ferns, d->capacity);
  KFN_LAUNCH_CHECK("reloc_distance_kernel");
  hipLaunchKernelGGL(reloc_select_kernel, dim3(1), dim3(TT), 0, st, dist, state, d->ferns, d->capacity, d->tries);
  KFN_LAUNCH_CHECK("reloc_select_kernel");
  return KFN_OK;
}

extern "C" int kfn_reloc_seed(const kfn_reloc_desc* d, kfn_reloc_state* state, kfn_track_state* track, const double* key_poses,
                              void* stream) {
  const char* who = "kfn_reloc_seed";
  const int rc = checked_reloc(d, who);
  if (rc != KFN_OK) return rc;
  KFN_REQUIRE(state && track && key_poses, "%s: null buffer (state, track and key_poses are required)", who);
  KFN_REQUIRE((((uintptr_t)state | (uintptr_t)track | (uintptr_t)key_poses) & 7) == 0, "%s: state, track and key_poses must be 8-byte aligned",
              who);
  hipLaunchKernelGGL(reloc_seed_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), state, track, key_poses, d->capacity,
                     d->tries);
  KFN_LAUNCH_CHECK("reloc_seed_kernel");
  return KFN_OK;
}

extern "C" int kfn_reloc_settle(const kfn_reloc_desc* d, kfn_reloc_state* state, kfn_track_state* track, const uint8_t* code, uint8_t* codes,
                                double* key_poses, float* pose_rows, double* trajectory, int32_t* reloc_rows, void* stream) {
  const char* who = "kfn_reloc_settle";
  const int rc = checked_reloc(d, who);
  if (rc != KFN_OK) return rc;
  KFN_REQUIRE(state && track && code && codes && key_poses && pose_rows && trajectory && reloc_rows,
              "%s: null buffer (state, track, code, codes, key_poses, pose_rows, trajectory and reloc_rows are required)", who);
  KFN_REQUIRE((((uintptr_t)state | (uintptr_t)track | (uintptr_t)key_poses | (uintptr_t)trajectory) & 7) == 0 &&
                  (((uintptr_t)pose_rows | (uintptr_t)reloc_rows) & 3) == 0,
              "%s: state, track, key_poses and trajectory must be 8-byte aligned, pose_rows and reloc_rows 4-byte", who);
  KFN_REQUIRE(d->slot >= 0 && d->slot <= 65534, "%s: slot %d outside 0 .. 65534", who, d->slot);
  KFN_REQUIRE(d->traj_rows >= 1, "%s: traj_rows must be positive, got %d", who, d->traj_rows);
  KFN_REQUIRE(d->first == 0 || d->first == 1, "%s: first must be 0 or 1, got %d", who, d->first);
  KFN_REQUIRE(d->reloc_min_share >= 0.0f && d->reloc_min_share <= 1.0f, "%s: reloc_min_share must lie in 0 .. 1", who);
  KFN_REQUIRE(d->reloc_max_rms > 0.0f && d->reloc_max_rms <= 3.0e38f, "%s: reloc_max_rms must be positive and finite", who);
  SettleArgs a;
  a.rs = state; a.ts = track; a.code = code; a.codes = codes; a.key_poses = key_poses;
  a.pose_row = pose_rows + (long)d->slot * 12;
  a.trajectory = trajectory; a.rows = reloc_rows;
  a.ferns = d->ferns; a.capacity = d->capacity; a.tries = d->tries; a.harvest = d->harvest;
  a.n_rows = d->rows; a.traj_rows = d->traj_rows; a.first = d->first;
  a.min_share = (double)d->reloc_min_share; a.max_rms = (double)d->reloc_max_rms;
  hipLaunchKernelGGL(reloc_settle_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), a);
  KFN_LAUNCH_CHECK("reloc_settle_kernel");
  return KFN_OK;
}
