// bez_snapshot.h -- the copy kernel of env snapshots (include/bez_sim.h "Env snapshots"): whole envs between a sim's buffers and a snapshot
// of M rows, in one launch for a save and one for a restore.  The host side (what a section is, presence, the global words): bez_sim.hip.
//
// The snapshot is SoA over its rows in 32-bit words: column c of row r is snap[c * rows + r], a 64-bit item two columns (low, high).  A
// section is a run of columns that mirrors one buffer of the sim; the env side of a section is one of three layouts:
//   SNAP_COL    base[w * n + e]                  SoA words (the state, rew, episode, the reward terms, end bits, the actuator record)
//   SNAP_COL64  ((u64*)base)[(w / 2) * n + e]    SoA 64-bit items (reset, progress, timeout, randomize, nonfinite, the end counts)
//   SNAP_ROW    base[e * width + w]              row-major (obs, the parameter rows)
// A workgroup takes SNAP_TILE entries -- (env, row) pairs, range-checked once into LDS, an entry with either id out of range is skipped --
// and one chunk of columns (blockIdx.y): lane i of a wave works on entry i, so a wave's access on the snapshot side is one contiguous
// 256-byte piece of a column (a gather by row id in a restore with row ids) and on the env side a gather / scatter by env id, contiguous for
// the identity; a 64-bit item moves as one 8-byte access on the env side.  A row-major section is one chunk and goes through LDS, SNAP_STRIDE
// (odd) words per entry: the env side moves as whole rows (consecutive lanes, consecutive words), the snapshot side as columns, and the 64
// lanes of a column access hit 64 banks.  Workgroup (0, 0) also moves the sim-global device words.
#pragma once
#include <stdint.h>

#include "bez_kernels.h"

namespace bez {

enum : int { SNAP_COL = 0, SNAP_COL64 = 1, SNAP_ROW = 2 };
enum : int { SNAP_SKIP = 0, SNAP_COPY = 1, SNAP_DEFAULT = 2 };   // SNAP_DEFAULT (restore, parameter rows): the entry's envs take row dflt[]
constexpr int SNAP_TILE = 64, SNAP_THREADS = 256, SNAP_CHUNK = 32;
constexpr int SNAP_STRIDE = BEZ_NUM_OBS | 1;
constexpr int SNAP_MAX_SECTIONS = 20, SNAP_MAX_CHUNKS = 128, SNAP_GLOBALS = 4;
static_assert(BEZ_NUM_OBS < SNAP_STRIDE && BEZ_NUM_OBS_WALK < SNAP_STRIDE && BEZ_NL < SNAP_STRIDE, "a row-major section fits one staged row");

struct SnapSection {
  uint32_t* env;        // the sim's buffer
  uint32_t off;         // first column in the snapshot
  int width, kind, mode;
  int dflt;             // SNAP_DEFAULT: its row of SnapArgs::dflt
  int pad;
};
struct SnapChunk { int16_t sec, w0, nw, pad; };   // columns w0 .. w0 + nw - 1 of section sec (SNAP_COL64: whole items; SNAP_ROW: the section)
struct SnapArgs {
  uint32_t* snap; int rows;                      // the snapshot's columns
  int n;                                          // envs of the sim
  const int32_t *env_ids, *row_ids; int count;   // entry i: env env_ids[i] (null: i), row row_ids[i] (null: i)
  int nchunks;
  uint32_t* glob[SNAP_GLOBALS]; int glob_words[SNAP_GLOBALS];   // the sim-global device words (null: left alone) ...
  uint32_t* glob_snap;                                          // ... and where the snapshot keeps them, one after the other
  float dflt[BEZ_PARAM_COUNT][BEZ_NL];           // the default row of every parameter (SNAP_DEFAULT)
  SnapSection sec[SNAP_MAX_SECTIONS];
  SnapChunk chunk[SNAP_MAX_CHUNKS];
};

// SAVE: env -> snapshot; else snapshot -> env
template <bool SAVE>
__global__ void __launch_bounds__(SNAP_THREADS) snapshot_copy_kernel(SnapArgs A) {
  __shared__ int env[SNAP_TILE], row[SNAP_TILE];
  __shared__ uint32_t staged[SNAP_TILE * SNAP_STRIDE];
  const int i0 = blockIdx.x * SNAP_TILE, ni = min(SNAP_TILE, A.count - i0);
  for (int r = threadIdx.x; r < SNAP_TILE; r += SNAP_THREADS) {
    int e = -1, q = -1;
    if (r < ni) {
      e = A.env_ids ? A.env_ids[i0 + r] : i0 + r;
      q = A.row_ids ? A.row_ids[i0 + r] : i0 + r;
      if (e < 0 || e >= A.n || q < 0 || q >= A.rows) e = q = -1;   // before anything is indexed with either
    }
    env[r] = e; row[r] = q;
  }
  __syncthreads();
  if (blockIdx.x == 0 && blockIdx.y == 0) {
    uint32_t* kept = A.glob_snap;
    for (int g = 0; g < SNAP_GLOBALS; ++g) {
      if (A.glob[g])
        for (int k = threadIdx.x; k < A.glob_words[g]; k += SNAP_THREADS) {
          if (SAVE) kept[k] = A.glob[g][k]; else A.glob[g][k] = kept[k];
        }
      kept += A.glob_words[g];
    }
  }
  for (int c = blockIdx.y; c < A.nchunks; c += gridDim.y) {   // (uniform over the workgroup: the barriers below are reached by all)
    const SnapChunk C = A.chunk[c];
    const SnapSection& S = A.sec[C.sec];
    uint32_t* col0 = A.snap + (size_t)S.off * A.rows;
    if (S.kind == SNAP_COL) {
      for (int i = threadIdx.x; i < C.nw * SNAP_TILE; i += SNAP_THREADS) {
        const int w = C.w0 + i / SNAP_TILE, r = i % SNAP_TILE;
        if (env[r] < 0) continue;
        uint32_t* at_env = S.env + (size_t)w * A.n + env[r];
        uint32_t* at_snap = col0 + (size_t)w * A.rows + row[r];
        if (SAVE) *at_snap = *at_env; else *at_env = *at_snap;
      }
    } else if (S.kind == SNAP_COL64) {
      for (int i = threadIdx.x; i < (C.nw / 2) * SNAP_TILE; i += SNAP_THREADS) {
        const int item = C.w0 / 2 + i / SNAP_TILE, r = i % SNAP_TILE;
        if (env[r] < 0) continue;
        uint2* at_env = reinterpret_cast<uint2*>(S.env) + (size_t)item * A.n + env[r];
        uint32_t* lo = col0 + (size_t)(2 * item) * A.rows + row[r];
        uint32_t* hi = lo + A.rows;
        if (SAVE) { const uint2 v = *at_env; *lo = v.x; *hi = v.y; } else { *at_env = make_uint2(*lo, *hi); }
      }
    } else {
      const int W = S.width;
      __syncthreads();   // the staged rows of this workgroup's previous chunk have been read
      if (SAVE) {
        for (int i = threadIdx.x; i < ni * W; i += SNAP_THREADS) {
          const int r = i / W, k = i % W;
          if (env[r] >= 0) staged[r * SNAP_STRIDE + k] = S.env[(size_t)env[r] * W + k];
        }
      } else if (S.mode == SNAP_COPY) {
        for (int i = threadIdx.x; i < W * SNAP_TILE; i += SNAP_THREADS) {
          const int k = i / SNAP_TILE, r = i % SNAP_TILE;
          if (env[r] >= 0) staged[r * SNAP_STRIDE + k] = col0[(size_t)k * A.rows + row[r]];
        }
      }
      __syncthreads();
      if (SAVE) {
        for (int i = threadIdx.x; i < W * SNAP_TILE; i += SNAP_THREADS) {
          const int k = i / SNAP_TILE, r = i % SNAP_TILE;
          if (env[r] >= 0) col0[(size_t)k * A.rows + row[r]] = staged[r * SNAP_STRIDE + k];
        }
      } else if (S.mode == SNAP_COPY) {
        for (int i = threadIdx.x; i < ni * W; i += SNAP_THREADS) {
          const int r = i / W, k = i % W;
          if (env[r] >= 0) S.env[(size_t)env[r] * W + k] = staged[r * SNAP_STRIDE + k];
        }
      } else {   // the snapshot has no such rows: the default row (k is uniform, so the row is read with scalar loads)
        for (int k = 0; k < W; ++k) {
          const uint32_t v = __float_as_uint(A.dflt[S.dflt][k]);
          for (int r = threadIdx.x; r < ni; r += SNAP_THREADS)
            if (env[r] >= 0) S.env[(size_t)env[r] * W + k] = v;
        }
      }
    }
  }
}

}  // namespace bez
