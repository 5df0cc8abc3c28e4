// bez_sim.hip -- host side of the C ABI declared in include/bez_sim.h (libbez_sim.so) plus the small
// layout kernels (Isaac AoS tensors <-> the simulator's SoA state); the kernels that run forward kinematics
// outside the step: bez_dynamics.h.  gfx950 only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "bez_kernels.h"
#include "bez_dynamics.h"
#include "bez_snapshot.h"
#include "bez_dr_step.h"
#include "bez_launch.h"

using namespace bez;

namespace {

thread_local std::string g_create_error;
// every snapshot alive, of any sim: a restore takes a snapshot of another sim, so "is this handle alive" cannot be asked of one sim
std::mutex g_snapshots_mutex;
std::vector<const BezSnapshot*> g_snapshots;

}  // namespace

// (DrState: bez_kernels.h -- the step kernels read the frame counter and the observation-noise parameters)

struct BezSim {
  BezSimConfig cfg;
  int device = 0;
  int n = 0;
  int64_t obs_calls = 0;  // compute_observations passes so far (quirk Q1: only the first sees prev = zeros)
  uint64_t post_calls = 0, reset_calls = 0;  // keys of the shared goal draw (bez_walk / bez_orient)
  bool cleats = false, has_ball = true;
  int kernel = 0;  // fused-step kernel: 0 = by size (below), 3 = 8 role waves, four lanes per env (bez_step_ws8q.hip), 1 = 8 role waves, one lane per env (bez_kernel_ws8.h), 2 = one env per lane (bez_kernels.h)
  int quad_max_envs = 4096;  // 16 envs x the device's CUs: up to here the lane-group form runs in one round of workgroups
  int nb = BEZ_NB, nbe = BEZ_NBE, nobs = BEZ_NUM_OBS, nact = 2;  // robot bodies, exported body rows, obs width, actors per env
  std::string err;
  // sim-owned device memory: every buffer is made by dev_alloc_zeroed, which records its slot here; bez_sim_destroy frees the list
  std::vector<void**> owned;
  float* state = nullptr;       // SoA [F_COUNT][N]
  float* obs = nullptr;         // (N,54)
  float* rew = nullptr;         // (N)
  int64_t* reset = nullptr;     // (N)
  int64_t* progress = nullptr;  // (N)
  int64_t* timeout = nullptr;   // (N)
  uint32_t* episode = nullptr;  // (N)
  // Isaac-layout tensors, materialised by bez_sim_refresh_tensor
  float* root_states = nullptr;  // (N*2,13)
  float* dof_state = nullptr;    // (N*18,2)
  float* rigid_body = nullptr;   // (N*22,13)
  float* contact = nullptr;      // (N*22,3)
  float* targets_aos = nullptr;  // (N,18)
  float* prev_aos = nullptr;     // (N,3)
  float* feet_aos = nullptr;     // (N,8)
  float* goal_aos = nullptr;     // (N,2)
  float* dr[BEZ_PARAM_COUNT] = {};
  // device-side domain randomisation (bez_sim_set_randomization)
  bool dr_on = false;
  bool obs_noise_applied = false;  // the last post-physics launch added the observation noise itself (BEZ_FLAG_OBS_NOISE_IN_STEP)
  BezDrConfig drc = {};
  int64_t* randomize = nullptr;   // (N) randomize_buf, vec_task.py:247
  DrState* dr_state = nullptr;  // device: frame counter, frame of the last non-env randomisation, noise parameters
  float* dr_noise = nullptr;    // = dr_state->noise (BEZ_TENSOR_DR_NOISE)
  DrSnap* dr_snap = nullptr;    // device: the action-noise parameters / frame the NEXT step's action noise uses (written by the step kernels)
  float4* dr_pack = nullptr;    // device (N,18): {kp scale, kd scale, lower, upper} per joint, kept equal to the four dr[] arrays (null while none of them exists)
  bool gravity_uniform = false; // every row of dr[GRAVITY] holds the same vector (written by the randomisation kernel, not by the user)
  bool dr_prelaunched = false;  // bez_sim_dr_prelaunch ran the randomisation kernel of the coming step already
  float* goal_draw_dev = nullptr;            // [2] the goal of the current post-physics reset (bez_walk / bez_orient)
  unsigned long long* post_calls_dev = nullptr;  // device-resident call counter keying that draw (HIP-graph replay safe)
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  unsigned long long* stamps = nullptr;  // diagnostic builds only
  float* xhit = nullptr;                 // BEZ_FLAG_ALL_GROUND_SHAPES: records of the extra ground points (BEZ_NXPT x 8 floats per env)
  int64_t* nonfinite = nullptr;          // (N) trips of the non-finite guard per env (BEZ_TENSOR_NONFINITE_COUNT)
  unsigned long long* health = nullptr;  // BEZ_HEALTH_* bits (BEZ_TENSOR_HEALTH)
  unsigned long long* episode_stats = nullptr;  // one allocation: (8,N) i64 BEZ_EPISODE_END_COUNTS, (8,N) f32 BEZ_EPISODE_REWARD_TERMS,
                                                // (N) i32 BEZ_EPISODE_END_BITS (bez_kernels.h end_counts_of / reward_terms_of / end_bits_of)
  // external wrenches (bez_sim_apply_body_forces): the pending buffer (bez_kernels.h EXT_*: [link][component][env] + one word per env),
  // allocated by the first call, which also switches every later physics launch of this sim to the EXT kernel instantiations (sticky:
  // a graph captured after it keeps consuming what later apply calls leave)
  float* ext = nullptr;
  bool ext_on = false;
  // actuator tensors (BEZ_FLAG_DOF_FORCE), one allocation made when the flag is first set: the raw record of the step kernels
  // [substep][3][dof][env] (bez_kernels.h df_record), then the three Isaac-layout tensors bez_sim_refresh_actuator_tensors fills
  float* df_raw = nullptr;
  float* df_out = nullptr;   // (N*18) net joint force, (N*18) drive torque, (N*18) i32 status
  // dynamics tensors (bez_sim_get_dynamics_tensor allocates each on its first acquisition; bez_sim_refresh_dynamics_tensors fills them)
  float* jacobian = nullptr;     // (N*nb, 6, 24)
  float* mass_matrix = nullptr;  // (N, 24, 24)
  // query states (bez_query_state_create): the ones alive, and the one the query entry points read instead of the live state (null: none)
  std::vector<BezQueryState*> queries;
  BezQueryState* bound = nullptr;
  // env snapshots (bez_snapshot_create): the ones alive
  std::vector<BezSnapshot*> snapshots;
};

// A query state: `rows` rows of the fields the query kernels read, row-by-row copies of the parameter rows they read, and tensors of its
// own.  Every buffer is the owning sim's (dev_alloc_zeroed / dev_free); `shown` says which parameter copies the kernels are handed --
// the others they see as null pointers, the defaults -- and is decided by the last set or capture.
struct BezQueryState {
  BezSim* sim = nullptr;
  int rows = 0;
  float* state = nullptr;                 // SoA [QS_FIELDS][rows]
  float* param[QS_PARAMS] = {};           // (rows, QS_PARAM_WIDTH[p]) of BEZ_PARAM_* QS_PARAM_ID[p]
  bool shown[QS_PARAMS] = {};
  float* rigid_body = nullptr;            // (rows*nbe, 13)       allocated on first acquisition (bez_query_state_tensor), as the sim's
  float* jacobian = nullptr;              // (rows*nb, 6, 24)      dynamics tensors are
  float* mass_matrix = nullptr;           // (rows, 24, 24)
};

namespace {

int fail(BezSim* s, int code, const char* what, hipError_t e = hipSuccess) {
  char buf[512];
  if (e != hipSuccess) snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
  else snprintf(buf, sizeof(buf), "%s", what);
  if (s) s->err = buf; else g_create_error = buf;
  return code;
}
#define HIP_TRY(s, call) do { hipError_t _e = (call); if (_e != hipSuccess) return fail((s), -2, #call, _e); } while (0)
#define RC_TRY(call) do { if (int _rc = (call)) return _rc; } while (0)

// The one owner of device memory: allocates `bytes` into *slot, zeroes them (in stream order on `stream`; before the call returns
// without one) and records the slot in s->owned.  dev_free releases a buffer before the sim ends; bez_sim_destroy releases the rest.
template <typename T>
int dev_alloc_zeroed(BezSim* s, T** slot, size_t bytes, hipStream_t stream = nullptr) {
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) return fail(s, -4, "hipMalloc", e);
  *slot = (T*)p;
  s->owned.push_back((void**)slot);
  e = stream ? hipMemsetAsync(p, 0, bytes, stream) : hipMemset(p, 0, bytes);
  return e == hipSuccess ? 0 : fail(s, -2, "hipMemset", e);
}
template <typename T>
void dev_free(BezSim* s, T** slot) {
  s->owned.erase(std::remove(s->owned.begin(), s->owned.end(), (void**)slot), s->owned.end());
  (void)hipFree(*slot);
  *slot = nullptr;
}

// The one checked launch: `total` elements, one per thread, in workgroups of THREADS; an error becomes rc -2 and "<kernel> launch".
constexpr int TB = 256;
template <int THREADS, typename... P, typename... A>
int launch_checked(BezSim* s, const char* what, void (*kernel)(P...), size_t total, hipStream_t stream, A... args) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream, static_cast<P>(args)...);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(s, -2, what, e);
}
#define LAUNCH(s, kernel, total, stream, ...) launch_checked<TB>((s), #kernel " launch", kernel, (total), (stream), __VA_ARGS__)
// The sim's asset picks the instantiation of a kernel template <bool CL>: workgroups of THREADS lanes, each taking TILE consecutive envs
#define LAUNCH_ASSET_ROWS(s, rows, kernel, TILE, THREADS, stream, ...)                                                                            \
  ((s)->cleats ? launch_checked<THREADS>((s), #kernel " launch", kernel<true>, (size_t)(((rows) + (TILE) - 1) / (TILE)) * (THREADS), (stream), __VA_ARGS__) \
               : launch_checked<THREADS>((s), #kernel " launch", kernel<false>, (size_t)(((rows) + (TILE) - 1) / (TILE)) * (THREADS), (stream), __VA_ARGS__))
#define LAUNCH_ASSET(s, kernel, TILE, THREADS, stream, ...) LAUNCH_ASSET_ROWS(s, (s)->n, kernel, TILE, THREADS, stream, __VA_ARGS__)
// the same over the rows of a StateView (below): the live state's envs, or a query state's rows
#define LAUNCH_VIEW(s, v, kernel, TILE, THREADS, stream, ...) LAUNCH_ASSET_ROWS(s, (v).n, kernel, TILE, THREADS, stream, __VA_ARGS__)

// host copy of the reset-noise Philox (bez_kernels.h) for the per-call goal draw
void philox_host(uint32_t c[4], uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}
// bez_walk / bez_orient: reset_idx draws goal xy ~ U(-2,2)^2 and gives THE FIRST SAMPLE to every env it resets
// (walk_env.py:570-575): one draw per reset call, keyed by (seed, call counter, kind 0 = post_physics_step / 1 = explicit reset_idx)
void goal_draw(uint64_t seed, uint64_t counter, uint32_t kind, float out[2]) {
  uint32_t c[4] = {(uint32_t)counter, (uint32_t)(counter >> 32), 0x474f414cu, kind};
  philox_host(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  for (int k = 0; k < 2; ++k) out[k] = std::fmaf(4.0f, (float)(c[k] >> 8) * (1.0f / 16777216.0f), -2.0f);
}

// device twin of goal_draw(seed, counter, 0, out) with the counter in device memory: one thread, launched in front of every step
// that contains the post-physics of bez_walk / bez_orient.  A captured HIP graph replays kernel arguments verbatim, so a goal
// passed by value would repeat the captured horizon's 32 goals forever; the counter here advances on every replay.
__global__ void goal_draw_kernel(uint64_t seed, unsigned long long* counter, float* out) {
  const unsigned long long cnt = *counter;
  uint32_t c[4] = {(uint32_t)cnt, (uint32_t)(cnt >> 32), 0x474f414cu, 0u};
  bez::philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  out[0] = fmaf(4.0f, (float)(c[0] >> 8) * (1.0f / 16777216.0f), -2.0f);
  out[1] = fmaf(4.0f, (float)(c[1] >> 8) * (1.0f / 16777216.0f), -2.0f);
  *counter = cnt + 1;
}

// ---- device-side domain randomisation: what reset_idx's apply_randomizations call does (vec_task.py:505-725, kick_env.py:781-782),
// for the whole batch, in ONE workgroup in front of the step kernel (so that "did any env reset" and the frame counter need no
// grid-wide synchronisation): thread t looks after envs t, t + 1024, ...  The word map of an env's Philox draw, keyed by
// (seed, global env id, episode): 0 friction; 1..18 stiffness; 19..36 damping; 37..72 lower limits (pairs, Box-Muller); 73..108 upper.
using bez::dr::DrArgs;
constexpr int DR_THREADS = 1024;
constexpr int DR_LIST = 8192;
static_assert(sizeof(DrArgs) <= BEZ_DR_STEP_BYTES, "BezPpoDrStep blob of the C ABI too small");
__global__ void __launch_bounds__(DR_THREADS) dr_kernel(DrArgs A) {
  __shared__ int list[DR_LIST];
  __shared__ int nlist;
  bez::dr::dr_step(A, list, DR_LIST, &nlist);
}

// vec_task.py:544-618 noise lambdas: x += mean + std * N(0,1); 4 elements per thread from one Philox block (two Box-Muller pairs)
__global__ void dr_noise_kernel(const float* x, float* y, long long n, const DrState* __restrict__ st, const DrSnap* __restrict__ snap, int which, uint64_t seed,
                                int64_t env_off) {
  const long long i4 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i4 * 4 >= n) return;
  // observations: the live state (this step's randomisation has run); actions: the snapshot the last step left -- the same numbers as
  // the live state unless the coming step's randomisation kernel was launched early (bez_sim_dr_prelaunch)
  const float mean = which ? snap->mean : st->noise[0], sd = which ? snap->sd : st->noise[1];
  const unsigned long long frame = which ? ((unsigned long long)snap->frame_hi << 32 | snap->frame_lo) : st->frame;
  float z[4];
  bez::dr_noise_quad(seed, env_off, frame, which, i4, z);   // (shared with the step kernels' observation copy-out: same bits)
  for (int k = 0; k < 4; ++k) if (i4 * 4 + k < n) y[i4 * 4 + k] = x[i4 * 4 + k] + fmaf(z[k], sd, mean);
}

__global__ void dr_repack_kernel(float4* pack, const float* kp, const float* kd, const float* lower, const float* upper, size_t total) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int j = (int)(i % BEZ_ND);
  pack[i] = make_float4(kp ? kp[i] : 1.f, kd ? kd[i] : 1.f, lower ? lower[i] : (float)BEZ_DOF_LOWER[j], upper ? upper[i] : (float)BEZ_DOF_UPPER[j]);
}
// (re)builds the packed copy from the four per-env arrays; called whenever one of them was written from outside the randomisation kernel
int repack_dr(BezSim* s, hipStream_t stream) {
  const bool any = s->dr[BEZ_PARAM_KP_SCALE] || s->dr[BEZ_PARAM_KD_SCALE] || s->dr[BEZ_PARAM_DOF_LOWER] || s->dr[BEZ_PARAM_DOF_UPPER];
  if (!any) {
    if (s->dr_pack) { HIP_TRY(s, hipStreamSynchronize(stream)); dev_free(s, &s->dr_pack); }
    return 0;
  }
  const size_t total = (size_t)s->n * BEZ_ND;
  if (!s->dr_pack) RC_TRY(dev_alloc_zeroed(s, &s->dr_pack, total * sizeof(float4), stream));
  return LAUNCH(s, dr_repack_kernel, total, stream, s->dr_pack, s->dr[BEZ_PARAM_KP_SCALE], s->dr[BEZ_PARAM_KD_SCALE], s->dr[BEZ_PARAM_DOF_LOWER],
                s->dr[BEZ_PARAM_DOF_UPPER], total);
}

DrArgs make_dr_args(const BezSim* s, bool first) {
  DrArgs A;
  A.c = s->drc; A.n = s->n; A.first = first ? 1 : 0; A.seed = s->cfg.seed; A.env_off = s->cfg.env_id_offset;
  A.plane_friction = s->cfg.plane_friction;
  for (int k = 0; k < 3; ++k) A.gravity[k] = s->cfg.gravity[k];
  A.reset = s->reset; A.episode = s->episode; A.randomize = s->randomize; A.st = s->dr_state; A.snap = s->dr_snap;
  A.friction = s->dr[BEZ_PARAM_FRICTION]; A.kp = s->dr[BEZ_PARAM_KP_SCALE]; A.kd = s->dr[BEZ_PARAM_KD_SCALE];
  A.lower = s->dr[BEZ_PARAM_DOF_LOWER]; A.upper = s->dr[BEZ_PARAM_DOF_UPPER]; A.gravity_rows = s->dr[BEZ_PARAM_GRAVITY];
  A.pack = s->dr_pack;
  return A;
}
void launch_dr(BezSim* s, bool first, hipStream_t stream) {
  dr_kernel<<<1, DR_THREADS, 0, stream>>>(make_dr_args(s, first));
}

Params make_params(const BezSim* s, const float* actions) {
  const BezSimConfig& c = s->cfg;
  Params P;
  std::memset(&P, 0, sizeof(P));
  P.n = s->n; P.substeps = c.substeps; P.max_len = c.max_episode_length;
  P.use_prev = (!(c.flags & BEZ_FLAG_IMU_PREV_ALIAS) || s->obs_calls == 0) ? 1 : 0;
  P.lean = 0;  // set by launch_step for the fused step only
  P.dt = c.dt; P.h = c.dt / (float)c.substeps; P.inv_h = 1.0f / P.h;
  {
    float igx = c.goal[0] - c.ball_init[0], igy = c.goal[1] - c.ball_init[1];
    float ign = std::sqrt(igx * igx + igy * igy);
    P.ang_init = std::atan2(igy / ign, igx / ign);
  }
  for (int i = 0; i < 3; ++i) P.g[i] = c.gravity[i];
  P.kp = c.kp; P.kd = c.kd; P.armature = c.armature; P.effort = c.effort; P.vel_limit = c.vel_limit;
  P.jfric = c.joint_friction; P.mu = c.plane_friction; P.clip = c.clip_actions;
  for (int i = 0; i < 7; ++i) { P.bez_init[i] = c.bez_init[i]; P.ball_init[i] = c.ball_init[i]; }
  P.goal[0] = c.goal[0]; P.goal[1] = c.goal[1];
  P.kn = c.contact_kn; P.cn = c.contact_cn; P.ct = c.contact_ct; P.veps = c.contact_veps;
  P.bkn = c.ball_kn > 0.f ? c.ball_kn : c.contact_kn; P.bcn = c.ball_cn > 0.f ? c.ball_cn : c.contact_cn;
  P.lim_k = c.limit_k; P.lim_d = c.limit_d; P.jf_veps = c.jfric_veps; P.ball_damp = c.ball_ang_damping;
  P.self_kn = c.self_kn; P.self_cn = c.self_cn;
  P.cf_w = (c.flags & BEZ_FLAG_CF_LAST_SUBSTEP) ? 1.0f : 1.0f / (float)c.substeps;
  P.task = c.task; P.nobs = s->nobs; P.goal_angle = c.goal_angle;
  P.goal_draw[0] = c.goal[0]; P.goal_draw[1] = c.goal[1];
  P.flags = c.flags; P.seed = c.seed; P.env_off = c.env_id_offset;
  P.state = s->state; P.obs = s->obs; P.rew = s->rew; P.reset = s->reset; P.progress = s->progress;
  P.timeout = s->timeout; P.episode = s->episode; P.actions = actions;
  P.dr_friction = s->dr[BEZ_PARAM_FRICTION]; P.dr_kp = s->dr[BEZ_PARAM_KP_SCALE]; P.dr_kd = s->dr[BEZ_PARAM_KD_SCALE];
  P.dr_mass = s->dr[BEZ_PARAM_MASS_SCALE]; P.dr_gravity = s->dr[BEZ_PARAM_GRAVITY];
  P.dr_lower = s->dr[BEZ_PARAM_DOF_LOWER]; P.dr_upper = s->dr[BEZ_PARAM_DOF_UPPER];
  P.dr_pack = s->dr_pack; P.dr_gravity_uniform = (s->dr[BEZ_PARAM_GRAVITY] && s->gravity_uniform) ? 1 : 0;
  P.stamps = s->stamps;
  P.nonfinite = s->nonfinite; P.health = s->health;
  P.episode_stats = s->episode_stats;
  P.xhit = (c.flags & BEZ_FLAG_ALL_GROUND_SHAPES) ? s->xhit : nullptr;
  P.ext = s->ext;
  return P;
}
// "The state the queries read", defined once: the SoA state, its row count, the four parameter rows over those rows (null: the defaults)
// and whether its rigid-body rows end with a ball.  live_view: the sim's own state; view_of: a query state; query_view: what the query
// entry points launch on -- the bound query state, else the live state.  Nothing but those entry points asks query_view.
struct StateView { const float *st, *mass_scale, *gravity_rows, *lower, *upper; int n; bool has_ball; };
StateView live_view(const BezSim* s) {
  return {s->state, s->dr[BEZ_PARAM_MASS_SCALE], s->dr[BEZ_PARAM_GRAVITY], s->dr[BEZ_PARAM_DOF_LOWER], s->dr[BEZ_PARAM_DOF_UPPER], s->n, s->has_ball};
}
StateView view_of(const BezQueryState* q) {
  static_assert(QS_PARAM_ID[0] == BEZ_PARAM_MASS_SCALE && QS_PARAM_ID[1] == BEZ_PARAM_GRAVITY && QS_PARAM_ID[2] == BEZ_PARAM_DOF_LOWER &&
                QS_PARAM_ID[3] == BEZ_PARAM_DOF_UPPER, "the order of a StateView's parameter rows");
  auto row = [&](int p) -> const float* { return q->shown[p] ? q->param[p] : nullptr; };
  return {q->state, row(0), row(1), row(2), row(3), q->rows, q->sim->has_ball};
}
StateView query_view(const BezSim* s) { return s->bound ? view_of(s->bound) : live_view(s); }
DynArgs dyn_args(const BezSim* s, const StateView& v) {
  const BezSimConfig& c = s->cfg;
  return {v.st, v.mass_scale, v.gravity_rows, v.n, c.flags, c.armature, {c.gravity[0], c.gravity[1], c.gravity[2]}};
}
bool has_dr(const BezSim* s) {
  for (int i = 0; i < BEZ_PARAM_COUNT; ++i) if (s->dr[i]) return true;
  return false;
}

// ---------------------------------------------------------------- layout kernels

// KickEnv.reset_idx for listed envs (or all when ids == nullptr)
__global__ void reset_kernel(Params P, const int32_t* ids, int count) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  int e = ids ? ids[t] : t;
  if (e < 0 || e >= P.n) return;
  EnvState S;
  float target[BEZ_ND];
  CfOut co;
  co.base = P.state + (size_t)F_CF * P.n + e; co.n = P.n;
  uint32_t episode = P.episode[e];
  env_reset(P, S, target, co, episode, P.env_off + e);  // also zeroes the env's contact-force rows
  P.episode[e] = episode;
  store_state(P.state, P.n, e, S);
  for (int j = 0; j < BEZ_ND; ++j) P.state[(size_t)(F_TARGET + j) * P.n + e] = target[j];
  if (P.task != BEZ_TASK_KICK) { P.state[(size_t)F_GOAL * P.n + e] = P.goal_draw[0]; P.state[(size_t)(F_GOAL + 1) * P.n + e] = P.goal_draw[1]; }
  P.progress[e] = 0;  // kick_env.py:849-850
  P.reset[e] = 0;
}

__global__ void init_misc_kernel(float* state, int n, float gx, float gy) {
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  state[(size_t)F_GOAL * n + e] = gx; state[(size_t)(F_GOAL + 1) * n + e] = gy;  // walk_env.py:143 self.goal
  for (int i = 0; i < 3; ++i) state[(size_t)(F_PREV + i) * n + e] = 0.f;  // kick_env.py:183
  for (int i = 0; i < 8; ++i) state[(size_t)(F_FEET + i) * n + e] = -1.f; // kick_env.py:185
}

__global__ void refresh_root_kernel(const float* __restrict__ st, float* __restrict__ out, int n, int nact) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int w = 13 * nact;  // robot row (+ ball row)
  if (t >= n * w) return;
  int e = t / w, k = t % w;
  int f = (k < 13) ? (F_ROOT_POS + k) : (F_BALL_POS + (k - 13));
  out[t] = st[(size_t)f * n + e];
}
__global__ void refresh_dof_kernel(const float* __restrict__ st, float* __restrict__ out, int n) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * BEZ_ND * 2) return;
  int e = t / (BEZ_ND * 2), k = t % (BEZ_ND * 2);
  int j = k >> 1;
  out[t] = st[(size_t)((k & 1) ? (F_QD + j) : (F_Q + j)) * n + e];
}
__global__ void refresh_rows_kernel(const float* __restrict__ st, float* __restrict__ out, int n, int field0, int width) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * width) return;
  int e = t / width, k = t % width;
  out[t] = st[(size_t)(field0 + k) * n + e];
}
__global__ void scatter_rows_kernel(float* __restrict__ st, const float* __restrict__ in, int n, int field0, int width) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * width) return;
  int e = t / width, k = t % width;
  st[(size_t)(field0 + k) * n + e] = in[t];
}

// gym.set_actor_root_state_tensor_indexed
__global__ void set_root_indexed_kernel(float* __restrict__ st, const float* __restrict__ src, const int32_t* __restrict__ ids, int count, int n, int nact) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count * 13) return;
  int a = ids[t / 13], k = t % 13;
  if (a < 0 || a >= n * nact) return;
  int e = a / nact;
  int f = (a % nact) ? (F_BALL_POS + k) : (F_ROOT_POS + k);
  st[(size_t)f * n + e] = src[(size_t)a * 13 + k];
}
// gym.set_dof_state_tensor_indexed (actor ids of robot actors: env*2)
__global__ void set_dof_indexed_kernel(float* __restrict__ st, const float* __restrict__ src, const int32_t* __restrict__ ids, int count, int n, int nact) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count * BEZ_ND * 2) return;
  int a = ids[t / (BEZ_ND * 2)], k = t % (BEZ_ND * 2);
  if (a < 0 || a >= n * nact || (a % nact)) return;
  int e = a / nact, j = k >> 1;
  st[(size_t)((k & 1) ? (F_QD + j) : (F_Q + j)) * n + e] = src[((size_t)e * BEZ_ND + j) * 2 + (k & 1)];
}
__global__ void set_target_indexed_kernel(float* __restrict__ st, const float* __restrict__ src, const int32_t* __restrict__ ids, int count, int n, int nact) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count * BEZ_ND) return;
  int a = ids[t / BEZ_ND], j = t % BEZ_ND;
  if (a < 0 || a >= n * nact || (a % nact)) return;
  int e = a / nact;
  st[(size_t)(F_TARGET + j) * n + e] = src[(size_t)e * BEZ_ND + j];
}

// bez_sim_refresh_actuator_tensors: mean over the substeps of the two torques, OR of the status words, non-finite -> 0, [dof][env] -> (N*18)
__global__ void refresh_actuator_kernel(const float* __restrict__ raw, float* __restrict__ out, int n, int substeps) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * BEZ_ND) return;
  const int d = t / n, e = t % n;   // (coalesced reads of the record; the stores are strided by 18 words)
  const size_t plane = (size_t)BEZ_ND * n;
  float drive = 0.f, net = 0.f;
  uint32_t bits = 0u;
  for (int s = 0; s < substeps; ++s) {
    const float* r = raw + (size_t)s * 3 * plane + (size_t)d * n + e;
    drive += r[0]; net += r[plane]; bits |= __float_as_uint(r[2 * plane]);
  }
  const float w = 1.0f / (float)substeps;
  const size_t o = (size_t)e * BEZ_ND + d, total = (size_t)n * BEZ_ND;
  out[o] = finite_or(net * w, 0.f);
  out[total + o] = finite_or(drive * w, 0.f);
  reinterpret_cast<int32_t*>(out)[2 * total + o] = (int32_t)(bits & 15u);
}
// the buffers that only a flag needs, on its first use (bez_sim_create and bez_sim_set_flags)
int ensure_flag_buffers(BezSim* s, uint32_t flags) {
  (void)hipSetDevice(s->device);
  if ((flags & BEZ_FLAG_ALL_GROUND_SHAPES) && !s->xhit) RC_TRY(dev_alloc_zeroed(s, &s->xhit, (size_t)s->n * BEZ_NXPT * 8 * sizeof(float)));
  if ((flags & BEZ_FLAG_DOF_FORCE) && !s->df_raw) {
    const size_t plane = (size_t)s->n * BEZ_ND, raw = (size_t)s->cfg.substeps * 3 * plane;
    RC_TRY(dev_alloc_zeroed(s, &s->df_raw, (raw + 3 * plane) * sizeof(float)));
    s->df_out = s->df_raw + raw;
  }
  return 0;
}

// ---------------------------------------------------------------- the tensor table: all the host side knows about a BezTensor.  A new tensor
// is one BezSim member, one enum value in include/bez_sim.h and one row here; create, get_tensor, refresh_tensor and the dense setters read it.
enum : int { PER_ENV = -1, PER_ACTOR = -2, PER_BODY = -3, PER_DOF = -4 };   // row rules: N, N * actors, N * exported bodies, N * 18 (>= 0: that many)
constexpr int COLS_OBS = -1;                                                // column rule: the task's observation width
enum Refresh { LIVE, ROWS, ROOT_KERNEL, DOF_KERNEL, RIGID_BODY_KERNEL };    // LIVE: written in place, a refresh is a no-op
struct TensorRow {
  int id;                      // its own index (checked below)
  void** (*slot)(BezSim*);     // the member that holds it
  int dtype, rows, cols;       // shape (rows, cols); cols 0: one-dimensional
  bool alloc;                  // bez_sim_create allocates it, for the largest layout (2 actors, BEZ_NBE_MAX bodies, BEZ_NUM_OBS columns)
  Refresh refresh;
  int field0;                  // ROWS: the env's row is the state fields field0 .. field0 + (elements per env) - 1
};
#define SLOT(member) [](BezSim* s) -> void** { return (void**)&s->member; }
constexpr TensorRow TENSORS[] = {
    {BEZ_TENSOR_ROOT_STATE, SLOT(root_states), BEZ_DTYPE_F32, PER_ACTOR, 13, true, ROOT_KERNEL, 0},
    {BEZ_TENSOR_DOF_STATE, SLOT(dof_state), BEZ_DTYPE_F32, PER_DOF, 2, true, DOF_KERNEL, 0},
    {BEZ_TENSOR_RIGID_BODY_STATE, SLOT(rigid_body), BEZ_DTYPE_F32, PER_BODY, 13, true, RIGID_BODY_KERNEL, 0},
    {BEZ_TENSOR_NET_CONTACT_FORCE, SLOT(contact), BEZ_DTYPE_F32, PER_BODY, 3, true, ROWS, F_CF},
    {BEZ_TENSOR_OBS, SLOT(obs), BEZ_DTYPE_F32, PER_ENV, COLS_OBS, true, LIVE, 0},
    {BEZ_TENSOR_REW, SLOT(rew), BEZ_DTYPE_F32, PER_ENV, 0, true, LIVE, 0},
    {BEZ_TENSOR_RESET, SLOT(reset), BEZ_DTYPE_I64, PER_ENV, 0, true, LIVE, 0},
    {BEZ_TENSOR_PROGRESS, SLOT(progress), BEZ_DTYPE_I64, PER_ENV, 0, true, LIVE, 0},
    {BEZ_TENSOR_TIMEOUT, SLOT(timeout), BEZ_DTYPE_I64, PER_ENV, 0, true, LIVE, 0},
    {BEZ_TENSOR_DOF_TARGET, SLOT(targets_aos), BEZ_DTYPE_F32, PER_ENV, BEZ_ND, true, ROWS, F_TARGET},
    {BEZ_TENSOR_PREV_LIN_VEL, SLOT(prev_aos), BEZ_DTYPE_F32, PER_ENV, 3, true, ROWS, F_PREV},
    {BEZ_TENSOR_FEET, SLOT(feet_aos), BEZ_DTYPE_F32, PER_ENV, 8, true, ROWS, F_FEET},
    {BEZ_TENSOR_GOAL, SLOT(goal_aos), BEZ_DTYPE_F32, PER_ENV, 2, true, ROWS, F_GOAL},
    {BEZ_TENSOR_RANDOMIZE_BUF, SLOT(randomize), BEZ_DTYPE_I64, PER_ENV, 0, true, LIVE, 0},
    {BEZ_TENSOR_DR_NOISE, SLOT(dr_noise), BEZ_DTYPE_F32, 4, 0, false, LIVE, 0},   // (inside dr_state)
    {BEZ_TENSOR_NONFINITE_COUNT, SLOT(nonfinite), BEZ_DTYPE_I64, PER_ENV, 0, true, LIVE, 0},
    {BEZ_TENSOR_HEALTH, SLOT(health), BEZ_DTYPE_I64, 1, 0, true, LIVE, 0},
};
#undef SLOT
constexpr bool tensor_ids_in_order() {
  for (int i = 0; i < BEZ_TENSOR_COUNT; ++i) if (TENSORS[i].id != i) return false;
  return true;
}
static_assert(sizeof(TENSORS) / sizeof(TENSORS[0]) == BEZ_TENSOR_COUNT && tensor_ids_in_order(), "one TENSORS row per BezTensor, in enum order");

// shape of tensor t in this sim -- or, `largest`, in the largest layout any sim has (what bez_sim_create allocates); returns the element count
size_t tensor_shape(const BezSim* s, const TensorRow& t, int64_t shape[2], bool largest = false) {
  const int64_t n = s->n, per_env = t.rows == PER_ACTOR ? (largest ? BEZ_NUM_ACTORS : s->nact) : t.rows == PER_BODY ? (largest ? BEZ_NBE_MAX : s->nbe) : t.rows == PER_DOF ? BEZ_ND : 1;
  shape[0] = t.rows < 0 ? n * per_env : t.rows;
  shape[1] = t.cols == COLS_OBS ? (largest ? BEZ_NUM_OBS : s->nobs) : t.cols;
  return (size_t)(shape[0] * (shape[1] ? shape[1] : 1));
}
size_t tensor_numel(const BezSim* s, const TensorRow& t, bool largest = false) { int64_t shape[2]; return tensor_shape(s, t, shape, largest); }

// the dense setters: an Isaac-layout (N, width) tensor back into the state fields its refresh reads
int scatter_rows(BezSim* s, int which, const float* src, void* stream, const char* bad_argument) {
  if (!s || !src) return fail(s, -1, bad_argument);
  const size_t total = tensor_numel(s, TENSORS[which]);
  return LAUNCH(s, scatter_rows_kernel, total, (hipStream_t)stream, s->state, src, s->n, TENSORS[which].field0, (int)(total / s->n));
}

// Kernel choice for launches that include the physics, fixed per sim at bez_sim_create from BEZ_SIM_KERNEL: "ws8q" = the 8-role-wave
// kernel in its lane-group form (four lanes per env, 16-env workgroups: bez_step_ws8q.hip), "ws8" = the one-lane form (bez_kernel_ws8.h,
// 64-env workgroups), "lane" = the one-env-per-lane reference kernel (bez_kernels.h).  Unset: by size -- the lane-group form while its
// workgroups fit the chip in one round (num_envs <= 16 x CUs = 4096 on MI355X: 23.6 against 27.6 us per step at 4096 envs, level for
// the cleats asset, 1 % ahead on the randomised PPO epoch), the one-lane form beyond (8192 envs: 27.9 us against 44.9, the lane-group
// form's second round; profiles/r06_ws_scale.txt).
int kernel_from_env() {
  const char* v = std::getenv("BEZ_SIM_KERNEL");
  if (!v) return 0;
  const std::string k(v);
  return k == "lane" ? 2 : (k == "ws8q" ? 3 : (k == "ws8" ? 1 : 0));
}

// PMC calibration: dword-per-lane coalesced read of `n` floats (the access shape of the step kernels' state loads)
__global__ void calib_read_kernel(const float* __restrict__ in, float* __restrict__ out, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  float acc = 0.f;
  for (; i < n; i += (size_t)gridDim.x * blockDim.x) acc += in[i];
  if (acc == 12345.678f) out[0] = acc;  // keeps the loads alive, never true for the calibration data
}
__global__ void calib_write_kernel(float* __restrict__ out, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] = 1.0f;
}

// Kernel instantiations: the default asset keeps its DR-free specialisation (the benchmark path); the cleats asset is always
// compiled with the per-env parameter loads (null pointers = defaults), which halves the number of variants to build.
template <bool PRE, bool SIM, bool POST>
int launch_step(BezSim* s, const float* actions, hipStream_t stream, bool obs_only = false) {
  Params P = make_params(s, actions);
  P.obs_only = obs_only ? 1 : 0;
  P.lean = (PRE && SIM && POST && !obs_only && (s->cfg.flags & BEZ_FLAG_LEAN_STEP) && (s->cfg.flags & BEZ_FLAG_IMU_PREV_ALIAS) && s->obs_calls > 0) ? 1 : 0;
  if (POST && !obs_only && s->dr_on) {   // reset_idx's apply_randomizations (kick_env.py:781-782), on the device
    if (!s->dr_prelaunched) launch_dr(s, false, stream);
    s->dr_prelaunched = false;           // (bez_sim_dr_prelaunch ran it for this step already, possibly on another stream: the caller joined)
  }
  // the observation noise of the randomisation inside this launch's copy-out (DR kernel variants only: has_dr is true once a
  // randomisation is set) -- bez_sim_add_dr_noise on the observation tensor is then a no-op
  const bool obs_noise = POST && !obs_only && s->dr_on && (s->cfg.flags & BEZ_FLAG_OBS_NOISE_IN_STEP) && s->drc.observations.enabled &&
                         true;                       // (an active randomisation always runs the kernel variants that carry the noise code)
  P.dr_state = s->dr_state; P.obs_noise = obs_noise ? 1 : 0;
  P.dr_snap = (POST && !obs_only && s->dr_on) ? s->dr_snap : nullptr;
  s->obs_noise_applied = obs_noise;
  if (POST && !obs_only && s->cfg.task != BEZ_TASK_KICK) {  // the reset inside this post_physics_step draws its goal on the device
    goal_draw_kernel<<<1, 1, 0, stream>>>(s->cfg.seed, s->post_calls_dev, s->goal_draw_dev);
    P.goal_dev = s->goal_draw_dev;
    s->post_calls++;
  }
  // an active randomisation runs the DR variants even when it owns no per-env array (null pointers = defaults): they carry the
  // observation noise and keep the action-noise snapshot
  const bool dr = has_dr(s) || s->cleats || s->dr_on;
  if constexpr (SIM && PRE == POST) {
    // urdfAsset.fixBaseLink (BEZ_FLAG_FIX_BASE): a test / debugging configuration of the reference (kick_env.py:287) -- served by the
    // one-env-per-lane kernel, which carries the "root acceleration = 0" branch; in the 8-role-wave kernel that branch costs the default
    // configuration 0.8 % (26.56 -> 26.78 us, same box: six more spilled VGPRs in a kernel at its 256-register ceiling)
    // (the same holds for the scenario harness's contact variants, BEZ_FLAG_ALL_GROUND_SHAPES / BEZ_FLAG_ANKLE_STOP: one-env-per-lane kernel only)
    const bool df = (s->cfg.flags & BEZ_FLAG_DOF_FORCE) != 0u;   // the recording instantiations (bez_step_*_df.hip)
    if (s->kernel != 2 && !(s->cfg.flags & (BEZ_FLAG_FIX_BASE | BEZ_FLAG_ALL_GROUND_SHAPES | BEZ_FLAG_ANKLE_STOP))) {
      const bool quad = s->kernel == 3 || (s->kernel == 0 && s->n <= s->quad_max_envs);
      if (df && quad) bez::launch_step_ws8q_df(P, s->df_raw, PRE, dr, s->cleats, stream, s->ext_on);
      else if (df) bez::launch_step_ws8_df(P, s->df_raw, PRE, dr, s->cleats, stream, s->ext_on);
      else if (quad) bez::launch_step_ws8q(P, PRE, dr, s->cleats, stream, s->ext_on);
      else bez::launch_step_ws8(P, PRE, dr, s->cleats, stream, s->ext_on);
      hipError_t e = hipGetLastError();
      if (e != hipSuccess) return fail(s, -2, "step_kernel_ws launch", e);
      if (POST) s->obs_calls += 1;
      return 0;
    }
  }
  bool recorded = false;
  if constexpr (SIM && PRE == POST) {
    if (s->cfg.flags & BEZ_FLAG_DOF_FORCE) { bez::launch_step_lane_df(P, s->df_raw, PRE, dr, s->cleats, stream, s->ext_on); recorded = true; }
  }
  if (!recorded) bez::launch_step_lane(P, PRE, SIM, POST, dr, s->cleats, stream, s->ext_on);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(s, -2, "step kernel launch", e);
  if (POST) s->obs_calls += 1;
  return 0;
}

}  // namespace

// =============================================================================================== C ABI
extern "C" {

int bez_sim_default_config(BezSimConfig* c, int32_t num_envs) {
  if (!c) return -1;
  std::memset(c, 0, sizeof(*c));
  c->abi_version = BEZ_SIM_ABI_VERSION;
  c->num_envs = num_envs;
  c->substeps = BEZ_DEFAULT_SUBSTEPS;
  c->dt = (float)BEZ_DEFAULT_DT;
  c->max_episode_length = (int32_t)(BEZ_DEFAULT_EPISODE_LENGTH_S / BEZ_DEFAULT_DT + 0.5);
  for (int i = 0; i < 3; ++i) c->gravity[i] = (float)BEZ_DEFAULT_GRAVITY[i];
  c->kp = (float)BEZ_DEFAULT_KP; c->kd = (float)BEZ_DEFAULT_KD; c->armature = (float)BEZ_DEFAULT_ARMATURE;
  c->effort = (float)BEZ_DEFAULT_EFFORT; c->vel_limit = (float)BEZ_DEFAULT_VEL_LIMIT;
  c->joint_friction = (float)BEZ_DEFAULT_JOINT_FRICTION; c->plane_friction = (float)BEZ_DEFAULT_PLANE_FRICTION;
  c->clip_actions = (float)BEZ_DEFAULT_CLIP_ACTIONS;
  for (int i = 0; i < 7; ++i) { c->bez_init[i] = (float)BEZ_DEFAULT_BEZ_INIT[i]; c->ball_init[i] = (float)BEZ_DEFAULT_BALL_INIT[i]; }
  c->goal[0] = (float)BEZ_DEFAULT_GOAL[0]; c->goal[1] = (float)BEZ_DEFAULT_GOAL[1];
  c->contact_kn = 2.0e4f; c->contact_cn = 20.0f; c->contact_ct = 1.0e3f; c->contact_veps = 0.01f;
  c->limit_k = 200.0f; c->limit_d = 2.0f; c->jfric_veps = 0.1f; c->ball_ang_damping = 0.5f;
  c->self_kn = 2.0e4f; c->self_cn = 5.0f;
  c->ball_kn = 0.0f; c->ball_cn = 0.0f;
  c->flags = BEZ_FLAG_IMU_PREV_ALIAS | BEZ_FLAG_NONFINITE_GUARD;
  c->seed = 42;
  c->env_id_offset = 0;
  return 0;
}

const char* bez_sim_last_error(const BezSim* sim) { return sim ? sim->err.c_str() : g_create_error.c_str(); }

/* Model variants that exist only in the CPU oracle (experiments that did not earn a kernel: DESIGN 3.1 / 6.1).  This library
 * has no kernel for them and says so instead of silently stepping the compliant model (include/bez_sim.h: BEZ_FLAG_HARD_CONTACT,
 * BEZ_FLAG_TGS_SOLVER, BezSimConfig.tune). */
static const char* oracle_only(uint32_t flags, const float* tune) {
  if (flags & BEZ_FLAG_HARD_CONTACT) return "BEZ_FLAG_HARD_CONTACT: rigid contact exists only in the CPU oracle; libbez_sim.so has no kernel for it";
  if (flags & BEZ_FLAG_TGS_SOLVER) return "BEZ_FLAG_TGS_SOLVER: the TGS-shaped solver exists only in the CPU oracle; libbez_sim.so has no kernel for it";
  // (round 6: the scenario harness's two contact variants run on the one-env-per-lane kernel -- for the asset they are defined for)
  if ((flags & (BEZ_FLAG_ANKLE_STOP | BEZ_FLAG_ALL_GROUND_SHAPES)) && (flags & (BEZ_FLAG_CLEATS | BEZ_FLAG_BOX_ASSET)))
    return "BEZ_FLAG_ANKLE_STOP / BEZ_FLAG_ALL_GROUND_SHAPES are defined for soccerbot_stl.urdf without cleats only (as in the CPU oracle); this asset has no kernel for them";
  // the actuator record of the scenario harness's two contact variants has no known-answer test yet (the ankle stop is a coupled limit of two
  // joints; the extra ground shapes only add link forces): refused rather than reported unchecked
  if ((flags & BEZ_FLAG_DOF_FORCE) && (flags & (BEZ_FLAG_ANKLE_STOP | BEZ_FLAG_ALL_GROUND_SHAPES)))
    return "BEZ_FLAG_DOF_FORCE with BEZ_FLAG_ANKLE_STOP / BEZ_FLAG_ALL_GROUND_SHAPES: the joint forces of these scenario variants are not validated; not served";
  if (tune) for (int i = 0; i < 24; ++i) if (tune[i] != 0.f) return "BezSimConfig.tune[]: knobs of the oracle-only solver variants; must be 0 for libbez_sim.so";
  return nullptr;
}

static void forget_snapshots(BezSim* s);   // (env snapshots, at the end of this file)
int bez_sim_destroy(BezSim* s) {
  if (!s) return 0;
  (void)hipSetDevice(s->device);
  for (void** slot : s->owned) (void)hipFree(*slot);   // (the buffers of the query states still alive among them)
  for (BezQueryState* q : s->queries) delete q;
  forget_snapshots(s);
  if (s->ev0) (void)hipEventDestroy(s->ev0);
  if (s->ev1) (void)hipEventDestroy(s->ev1);
  delete s;
  return 0;
}

// the device side of bez_sim_create: every buffer, then the state after KickEnv.__init__.  On an error the caller destroys the sim.
static int sim_init(BezSim* s) {
  const size_t n = (size_t)s->n;
  for (const TensorRow& t : TENSORS)
    if (t.alloc) RC_TRY(dev_alloc_zeroed(s, t.slot(s), tensor_numel(s, t, true) * (t.dtype == BEZ_DTYPE_I64 ? 8 : 4)));
  RC_TRY(dev_alloc_zeroed(s, &s->state, n * F_COUNT * sizeof(float)));
  RC_TRY(dev_alloc_zeroed(s, &s->episode, n * sizeof(uint32_t)));
  RC_TRY(dev_alloc_zeroed(s, &s->goal_draw_dev, 2 * sizeof(float)));
  RC_TRY(dev_alloc_zeroed(s, &s->post_calls_dev, sizeof(unsigned long long)));
  RC_TRY(dev_alloc_zeroed(s, &s->dr_state, sizeof(DrState)));
  s->dr_noise = s->dr_state->noise;
  RC_TRY(dev_alloc_zeroed(s, &s->dr_snap, sizeof(DrSnap)));
  RC_TRY(dev_alloc_zeroed(s, &s->episode_stats, BEZ_END_CAUSES * n * (sizeof(int64_t) + sizeof(float)) + n * sizeof(int32_t)));
  RC_TRY(ensure_flag_buffers(s, s->cfg.flags));
  (void)hipEventCreate(&s->ev0);
  (void)hipEventCreate(&s->ev1);
  // state after KickEnv.__init__: allocate_buffers (vec_task.py:226-249) then reset_idx(all) (kick_env.py:238)
  Params P = make_params(s, nullptr);
  goal_draw(s->cfg.seed, s->reset_calls++, 1, P.goal_draw);  // the reset_idx(all) that ends Kick/Walk/OrientEnv.__init__
  RC_TRY(LAUNCH(s, init_misc_kernel, n, nullptr, s->state, s->n, s->cfg.goal[0], s->cfg.goal[1]));
  RC_TRY(LAUNCH(s, reset_kernel, n, nullptr, P, (const int32_t*)nullptr, s->n));
  const hipError_t e = hipDeviceSynchronize();
  return e == hipSuccess ? 0 : fail(s, -2, "init kernels", e);
}

int bez_sim_create(const BezSimConfig* cfg, int device_id, BezSim** out) {
  if (!cfg || !out) return fail(nullptr, -1, "bez_sim_create: null argument");
  *out = nullptr;
  if (cfg->abi_version != BEZ_SIM_ABI_VERSION) return fail(nullptr, -1, "bez_sim_create: BezSimConfig.abi_version mismatch");
  if (cfg->num_envs <= 0) return fail(nullptr, -1, "bez_sim_create: num_envs must be > 0");
  if (cfg->substeps <= 0 || !(cfg->dt > 0.f)) return fail(nullptr, -1, "bez_sim_create: substeps and dt must be > 0");
  if (const char* why = oracle_only(cfg->flags, cfg->tune)) return fail(nullptr, -5, why);
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) return fail(nullptr, -3, "bez_sim_create: no HIP device available (the HIP path has no CPU fallback)", e);
  if (device_id < 0 || device_id >= ndev) return fail(nullptr, -1, "bez_sim_create: bad device id");
  e = hipSetDevice(device_id);
  if (e != hipSuccess) return fail(nullptr, -2, "hipSetDevice", e);
  BezSim* s = new (std::nothrow) BezSim();
  if (!s) return fail(nullptr, -4, "out of host memory");
  s->cfg = *cfg; s->device = device_id; s->n = cfg->num_envs;
  if (cfg->task < BEZ_TASK_KICK || cfg->task > BEZ_TASK_ORIENT) { delete s; return fail(nullptr, -1, "bez_sim_create: unknown task"); }
  s->cleats = (cfg->flags & BEZ_FLAG_CLEATS) != 0;
  s->kernel = kernel_from_env();
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && cus > 0) s->quad_max_envs = 16 * cus;
  }
  s->has_ball = cfg->task == BEZ_TASK_KICK;                    // walk_env.py / orient_env.py create no ball actor
  s->nb = s->cleats ? BEZ_NB_CL : BEZ_NB;
  s->nbe = s->nb + (s->has_ball ? 1 : 0);
  s->nact = s->has_ball ? 2 : 1;
  s->nobs = s->has_ball ? BEZ_NUM_OBS : BEZ_NUM_OBS_WALK;      // walk_env.py:104
  if (!s->has_ball) { s->cfg.ball_init[0] = 1000.0f; s->cfg.ball_init[1] = 0.0f; s->cfg.ball_init[2] = (float)BEZ_BALL_RADIUS; }  // parked out of reach
  if (int rc = sim_init(s)) { g_create_error = s->err; bez_sim_destroy(s); return rc; }
  *out = s;
  return 0;
}

int bez_sim_get_tensor(BezSim* s, int which, void** dev_ptr, int64_t shape[3], int* ndim, int* dtype) {
  if (!s || !dev_ptr || !shape || !ndim || !dtype) return fail(s, -1, "bez_sim_get_tensor: null argument");
  if (which < 0 || which >= BEZ_TENSOR_COUNT) return fail(s, -1, "bez_sim_get_tensor: unknown tensor id");
  const TensorRow& t = TENSORS[which];
  *dev_ptr = *t.slot(s); *dtype = t.dtype; *ndim = t.cols ? 2 : 1;
  tensor_shape(s, t, shape);
  return 0;
}

int bez_sim_get_episode_tensor(BezSim* s, int which, void** dev_ptr, int64_t shape[3], int* ndim, int* dtype) {
  if (!s || !dev_ptr || !shape || !ndim || !dtype) return fail(s, -1, "bez_sim_get_episode_tensor: null argument");
  const int64_t n = s->n;
  shape[0] = shape[1] = shape[2] = 0;
  switch (which) {   // (always live: the step kernels write them in place, there is nothing to refresh)
    case BEZ_EPISODE_END_COUNTS: *dev_ptr = s->episode_stats; shape[0] = BEZ_END_CAUSES; shape[1] = n; *ndim = 2; *dtype = BEZ_DTYPE_I64; break;
    case BEZ_EPISODE_REWARD_TERMS: *dev_ptr = s->episode_stats + BEZ_END_CAUSES * n; shape[0] = BEZ_END_CAUSES; shape[1] = n; *ndim = 2; *dtype = BEZ_DTYPE_F32; break;
    case BEZ_EPISODE_END_BITS: *dev_ptr = (float*)(s->episode_stats + BEZ_END_CAUSES * n) + BEZ_END_CAUSES * n; shape[0] = n; *ndim = 1; *dtype = BEZ_DTYPE_I32; break;
    default: return fail(s, -1, "bez_sim_get_episode_tensor: unknown tensor id");
  }
  return 0;
}

int bez_sim_refresh_tensor(BezSim* s, int which, void* stream_) {
  if (!s) return -1;
  hipStream_t stream = (hipStream_t)stream_;
  if (which < 0 || which >= BEZ_TENSOR_COUNT) return fail(s, -1, "bez_sim_refresh_tensor: unknown tensor id");
  const TensorRow& t = TENSORS[which];
  const int n = s->n;
  const size_t total = tensor_numel(s, t);
  float* out = (float*)*t.slot(s);
  switch (t.refresh) {
    case LIVE: return 0;
    case ROWS: return LAUNCH(s, refresh_rows_kernel, total, stream, s->state, out, n, t.field0, (int)(total / n));
    case ROOT_KERNEL: return LAUNCH(s, refresh_root_kernel, total, stream, s->state, out, n, s->nact);
    case DOF_KERNEL: return LAUNCH(s, refresh_dof_kernel, total, stream, s->state, out, n);
    case RIGID_BODY_KERNEL:
      return LAUNCH_ASSET(s, refresh_rigid_body_kernel, 64, 64, stream, s->state, out, n, (int)s->has_ball, s->cfg.flags);
  }
  return 0;
}

int bez_sim_set_actor_root_state_tensor_indexed(BezSim* s, const float* root_states_dev, const int32_t* ids, int32_t count, void* stream) {
  if (!s || !root_states_dev || (!ids && count > 0) || count < 0) return fail(s, -1, "set_actor_root_state_tensor_indexed: bad argument");
  if (count == 0) return 0;
  return LAUNCH(s, set_root_indexed_kernel, (size_t)count * 13, (hipStream_t)stream, s->state, root_states_dev, ids, count, s->n, s->nact);
}
int bez_sim_set_dof_state_tensor_indexed(BezSim* s, const float* dof_state_dev, const int32_t* ids, int32_t count, void* stream) {
  if (!s || !dof_state_dev || (!ids && count > 0) || count < 0) return fail(s, -1, "set_dof_state_tensor_indexed: bad argument");
  if (count == 0) return 0;
  return LAUNCH(s, set_dof_indexed_kernel, (size_t)count * BEZ_ND * 2, (hipStream_t)stream, s->state, dof_state_dev, ids, count, s->n, s->nact);
}
int bez_sim_set_dof_position_target_tensor(BezSim* s, const float* targets_dev, void* stream) {
  return scatter_rows(s, BEZ_TENSOR_DOF_TARGET, targets_dev, stream, "set_dof_position_target_tensor: bad argument");
}
int bez_sim_set_dof_position_target_tensor_indexed(BezSim* s, const float* targets_dev, const int32_t* ids, int32_t count, void* stream) {
  if (!s || !targets_dev || (!ids && count > 0) || count < 0) return fail(s, -1, "set_dof_position_target_tensor_indexed: bad argument");
  if (count == 0) return 0;
  return LAUNCH(s, set_target_indexed_kernel, (size_t)count * BEZ_ND, (hipStream_t)stream, s->state, targets_dev, ids, count, s->n, s->nact);
}
int bez_sim_set_net_contact_force_tensor(BezSim* s, const float* forces_dev, void* stream) {
  return scatter_rows(s, BEZ_TENSOR_NET_CONTACT_FORCE, forces_dev, stream, "set_net_contact_force_tensor: bad argument");
}
/* test hook used by the parity tests: writes prev_lin_vel (N,3) */
int bez_sim_set_prev_lin_vel_tensor(BezSim* s, const float* prev_dev, void* stream) {
  return scatter_rows(s, BEZ_TENSOR_PREV_LIN_VEL, prev_dev, stream, "set_prev_lin_vel_tensor: bad argument");
}
int bez_sim_set_flags(BezSim* s, uint32_t flags) {
  if (!s) return -1;
  const uint32_t asset = BEZ_FLAG_CLEATS | BEZ_FLAG_BOX_ASSET;  // the asset is fixed at creation (buffer shapes, kernel variant)
  const uint32_t merged = (flags & ~asset) | (s->cfg.flags & asset);
  if (const char* why = oracle_only(merged, nullptr)) return fail(s, -5, why);
  RC_TRY(ensure_flag_buffers(s, merged));
  s->cfg.flags = merged;
  return 0;
}

int bez_sim_get_actuator_tensor(BezSim* s, int which, void** dev_ptr, int64_t shape[3], int* ndim, int* dtype) {
  if (!s || !dev_ptr || !shape || !ndim || !dtype) return fail(s, -1, "bez_sim_get_actuator_tensor: null argument");
  if (!(s->cfg.flags & BEZ_FLAG_DOF_FORCE) || !s->df_out) return fail(s, -1, "bez_sim_get_actuator_tensor: BEZ_FLAG_DOF_FORCE is not set (the step kernels record no joint forces without it)");
  const size_t total = (size_t)s->n * BEZ_ND;
  shape[0] = (int64_t)total; shape[1] = shape[2] = 0; *ndim = 1;
  switch (which) {
    case BEZ_ACTUATOR_DOF_FORCE: *dev_ptr = s->df_out; *dtype = BEZ_DTYPE_F32; break;
    case BEZ_ACTUATOR_DRIVE_TORQUE: *dev_ptr = s->df_out + total; *dtype = BEZ_DTYPE_F32; break;
    case BEZ_ACTUATOR_STATUS: *dev_ptr = s->df_out + 2 * total; *dtype = BEZ_DTYPE_I32; break;
    default: return fail(s, -1, "bez_sim_get_actuator_tensor: unknown tensor id");
  }
  return 0;
}
int bez_sim_refresh_actuator_tensors(BezSim* s, void* stream) {
  if (!s) return -1;
  if (!(s->cfg.flags & BEZ_FLAG_DOF_FORCE) || !s->df_raw) return fail(s, -1, "bez_sim_refresh_actuator_tensors: BEZ_FLAG_DOF_FORCE is not set (the step kernels record no joint forces without it)");
  return LAUNCH(s, refresh_actuator_kernel, (size_t)s->n * BEZ_ND, (hipStream_t)stream, s->df_raw, s->df_out, s->n, s->cfg.substeps);
}
// ---- dynamics tensors: a table in the manner of TENSORS, with a third dimension and an allocation on first acquisition
struct DynamicsRow { int id; float** (*slot)(BezSim*); int per_env_bodies; int64_t d1, d2; };   // rows: N x robot bodies, or N
constexpr DynamicsRow DYNAMICS[] = {
    {BEZ_DYNAMICS_JACOBIAN, [](BezSim* s) -> float** { return &s->jacobian; }, 1, 6, 6 + BEZ_ND},
    {BEZ_DYNAMICS_MASS_MATRIX, [](BezSim* s) -> float** { return &s->mass_matrix; }, 0, 6 + BEZ_ND, 6 + BEZ_ND},
};
static_assert(sizeof(DYNAMICS) / sizeof(DYNAMICS[0]) == BEZ_DYNAMICS_COUNT && DYNAMICS[1].id == 1, "one DYNAMICS row per BezDynamicsTensor, in enum order");

int bez_sim_get_dynamics_tensor(BezSim* s, int which, void** dev_ptr, int64_t shape[3], int* ndim, int* dtype) {
  if (!s || !dev_ptr || !shape || !ndim || !dtype) return fail(s, -1, "bez_sim_get_dynamics_tensor: null argument");
  if (which < 0 || which >= BEZ_DYNAMICS_COUNT) return fail(s, -1, "bez_sim_get_dynamics_tensor: unknown tensor id");
  const DynamicsRow& t = DYNAMICS[which];
  shape[0] = (int64_t)s->n * (t.per_env_bodies ? s->nb : 1); shape[1] = t.d1; shape[2] = t.d2;
  float** slot = t.slot(s);
  if (!*slot) {   // the acquisition: the one place that allocates (and, through hipMemset, waits)
    (void)hipSetDevice(s->device);
    RC_TRY(dev_alloc_zeroed(s, slot, (size_t)(shape[0] * shape[1] * shape[2]) * sizeof(float)));
  }
  *dev_ptr = *slot; *ndim = 3; *dtype = BEZ_DTYPE_F32;
  return 0;
}
int bez_sim_refresh_dynamics_tensors(BezSim* s, uint32_t which_mask, void* stream) {
  if (!s) return -1;
  if (which_mask == 0u || (which_mask >> BEZ_DYNAMICS_COUNT)) return fail(s, -1, "bez_sim_refresh_dynamics_tensors: which_mask must be a non-empty set of (1u << BezDynamicsTensor) bits");
  float* J = (which_mask & (1u << BEZ_DYNAMICS_JACOBIAN)) ? s->jacobian : nullptr;
  float* M = (which_mask & (1u << BEZ_DYNAMICS_MASS_MATRIX)) ? s->mass_matrix : nullptr;
  if (((which_mask & (1u << BEZ_DYNAMICS_JACOBIAN)) && !J) || ((which_mask & (1u << BEZ_DYNAMICS_MASS_MATRIX)) && !M))
    return fail(s, -1, "bez_sim_refresh_dynamics_tensors: a requested tensor was never acquired (bez_sim_get_dynamics_tensor allocates it)");
  const StateView v = live_view(s);
  return LAUNCH_VIEW(s, v, refresh_dynamics_kernel, DYN_TILE, DYN_THREADS, (hipStream_t)stream, dyn_args(s, v), J, M);
}
int bez_sim_inverse_dynamics(BezSim* s, const float* udot_dev, uint32_t terms, float* out_dev, void* stream) {
  if (!s) return -1;
  if (terms == 0u || (terms & ~(uint32_t)BEZ_ID_ALL)) return fail(s, -1, "bez_sim_inverse_dynamics: terms must be a non-empty set of BEZ_ID_INERTIA | BEZ_ID_VELOCITY | BEZ_ID_GRAVITY");
  if (!out_dev) return fail(s, -1, "bez_sim_inverse_dynamics: out_dev is null");
  const StateView v = query_view(s);
  return LAUNCH_VIEW(s, v, inverse_dynamics_kernel, ID_TILE, ID_THREADS, (hipStream_t)stream, dyn_args(s, v), udot_dev, out_dev, terms);
}
int bez_sim_forward_dynamics(BezSim* s, const float* force_dev, uint32_t bias, uint32_t mode, float* out_dev, void* stream) {
  if (!s) return fail(s, -1, "bez_sim_forward_dynamics: sim is null");
  if (bias & ~(uint32_t)(BEZ_ID_VELOCITY | BEZ_ID_GRAVITY)) return fail(s, -1, "bez_sim_forward_dynamics: bias must be a subset of BEZ_ID_VELOCITY | BEZ_ID_GRAVITY");
  if (bias == 0u && !force_dev) return fail(s, -1, "bez_sim_forward_dynamics: bias is 0 and force_dev is null (nothing to solve for)");
  if (mode & ~(uint32_t)BEZ_FD_FIXED_BASE) return fail(s, -1, "bez_sim_forward_dynamics: mode must be 0 or BEZ_FD_FIXED_BASE");
  if (!out_dev) return fail(s, -1, "bez_sim_forward_dynamics: out_dev is null");
  const StateView v = query_view(s);
  return LAUNCH_VIEW(s, v, forward_dynamics_kernel, FD_TILE, FD_THREADS, (hipStream_t)stream, dyn_args(s, v), force_dev, out_dev, bias,
                     (int)(mode & BEZ_FD_FIXED_BASE));
}
int bez_sim_operational_space(BezSim* s, const BezOpSpaceParams* params, float* jac_dev, float* jminv_dev, float* w_dev, float* lambda_dev, void* stream) {
  if (!s) return fail(s, -1, "bez_sim_operational_space: sim is null");
  if (!params) return fail(s, -1, "bez_sim_operational_space: params is null");
  if (!jac_dev && !jminv_dev && !w_dev && !lambda_dev) return fail(s, -1, "bez_sim_operational_space: all four outputs are null (nothing to write)");
  const BezOpSpaceParams p = *params;
  if (p.mode & ~(uint32_t)BEZ_FD_FIXED_BASE) return fail(s, -1, "bez_sim_operational_space: mode must be 0 or BEZ_FD_FIXED_BASE");
  for (int c = 0; c < BEZ_IK_CHAINS; ++c)
    for (int k = 0; k < 3; ++k)
      if (!std::isfinite(p.offset[c][k])) return fail(s, -1, "bez_sim_operational_space: an offset is not finite");
  if ((p.mode & BEZ_FD_FIXED_BASE) && lambda_dev)
    return fail(s, -1, "bez_sim_operational_space: lambda_dev with BEZ_FD_FIXED_BASE (W_cc of a held root is singular by structure)");
  const StateView v = query_view(s);
  return LAUNCH_VIEW(s, v, operational_space_kernel, OS_TILE, OS_THREADS, (hipStream_t)stream, dyn_args(s, v), p, jac_dev, jminv_dev, w_dev, lambda_dev);
}
int bez_sim_centroidal(BezSim* s, float* state_dev, float* matrix_dev, void* stream) {
  if (!s) return fail(s, -1, "bez_sim_centroidal: sim is null");
  if (!state_dev && !matrix_dev) return fail(s, -1, "bez_sim_centroidal: state_dev and matrix_dev are both null (nothing to write)");
  const StateView v = query_view(s);
  return LAUNCH_VIEW(s, v, centroidal_kernel, CM_TILE, CM_THREADS, (hipStream_t)stream, dyn_args(s, v), state_dev, matrix_dev);
}
int bez_sim_body_accelerations(BezSim* s, const float* udot_dev, uint32_t terms, int32_t space, float* out_dev, void* stream) {
  if (!s) return fail(s, -1, "bez_sim_body_accelerations: sim is null");
  if (terms == 0u || (terms & ~(uint32_t)BEZ_ACC_ALL)) return fail(s, -1, "bez_sim_body_accelerations: terms must be a non-empty set of BEZ_ACC_UDOT | BEZ_ACC_VELOCITY | BEZ_ACC_GRAVITY");
  if (space != BEZ_SPACE_ENV && space != BEZ_SPACE_LOCAL) return fail(s, -1, "bez_sim_body_accelerations: space must be BEZ_SPACE_ENV or BEZ_SPACE_LOCAL");
  if (!out_dev) return fail(s, -1, "bez_sim_body_accelerations: out_dev is null");
  const StateView v = query_view(s);
  return LAUNCH_VIEW(s, v, body_accelerations_kernel, ACC_TILE, ACC_THREADS, (hipStream_t)stream, dyn_args(s, v), udot_dev, out_dev, terms, (int)space);
}
int bez_sim_generalized_forces(BezSim* s, const float* forces_dev, const float* torques_dev, const float* positions_dev, int32_t space,
                               float* out_dev, void* stream) {
  if (!s) return fail(s, -1, "bez_sim_generalized_forces: sim is null");
  if (space & ~(int32_t)(BEZ_SPACE_LOCAL | BEZ_GF_AT_ORIGIN)) return fail(s, -1, "bez_sim_generalized_forces: space must be BEZ_SPACE_ENV or BEZ_SPACE_LOCAL, optionally | BEZ_GF_AT_ORIGIN");
  if ((space & BEZ_GF_AT_ORIGIN) && positions_dev) return fail(s, -1, "bez_sim_generalized_forces: BEZ_GF_AT_ORIGIN needs positions_dev == NULL");
  if (!forces_dev && !torques_dev) return fail(s, -1, "bez_sim_generalized_forces: forces_dev and torques_dev are both null (nothing to map)");
  if (!out_dev) return fail(s, -1, "bez_sim_generalized_forces: out_dev is null");
  const StateView v = query_view(s);
  return LAUNCH_VIEW(s, v, generalized_forces_kernel, GF_TILE, GF_THREADS, (hipStream_t)stream, dyn_args(s, v), forces_dev, torques_dev, positions_dev,
                     (int)space, (int)v.has_ball, out_dev);
}
int bez_sim_limb_ik(BezSim* s, const float* targets_dev, const BezIkParams* params, float* q_out_dev, float* err_out_dev, void* stream) {
  if (!s) return fail(s, -1, "bez_sim_limb_ik: sim is null");
  if (!targets_dev) return fail(s, -1, "bez_sim_limb_ik: targets_dev is null");
  if (!params) return fail(s, -1, "bez_sim_limb_ik: params is null");
  if (!q_out_dev && !err_out_dev) return fail(s, -1, "bez_sim_limb_ik: q_out_dev and err_out_dev are both null (nothing to write)");
  const BezIkParams& p = *params;
  if (p.iters < 0 || p.iters > BEZ_IK_MAX_ITERS) return fail(s, -1, "bez_sim_limb_ik: iters must be in 0 .. BEZ_IK_MAX_ITERS");
  if (!(std::isfinite(p.damping) && p.damping > 0.f)) return fail(s, -1, "bez_sim_limb_ik: damping must be a positive finite number");
  if (std::isnan(p.max_step)) return fail(s, -1, "bez_sim_limb_ik: max_step is NaN (<= 0 means no step limit)");
  for (int c = 0; c < BEZ_IK_CHAINS; ++c) {
    for (int k = 0; k < 2; ++k)
      if (!(std::isfinite(p.weight[c][k]) && p.weight[c][k] >= 0.f)) return fail(s, -1, "bez_sim_limb_ik: a weight is negative or not finite");
    for (int k = 0; k < 3; ++k)
      if (!std::isfinite(p.offset[c][k])) return fail(s, -1, "bez_sim_limb_ik: an offset is not finite");
  }
  if (p.space != BEZ_IK_SPACE_ENV && p.space != BEZ_IK_SPACE_ROOT) return fail(s, -1, "bez_sim_limb_ik: space must be BEZ_IK_SPACE_ENV or BEZ_IK_SPACE_ROOT");
  const StateView v = query_view(s);
  return LAUNCH_VIEW(s, v, limb_ik_kernel, IK_TILE, IK_THREADS, (hipStream_t)stream, dyn_args(s, v), v.lower, v.upper,
                     targets_dev, p, q_out_dev, err_out_dev);
}
int bez_sim_proximity(BezSim* s, float* ground_dev, float* ball_dev, float* pairs_dev, void* stream) {
  if (!s) return fail(s, -1, "bez_sim_proximity: sim is null");
  if (!ground_dev && !ball_dev && !pairs_dev) return fail(s, -1, "bez_sim_proximity: ground_dev, ball_dev and pairs_dev are all null (nothing to write)");
  const StateView v = query_view(s);
  return LAUNCH_VIEW(s, v, proximity_kernel, PX_TILE, PX_THREADS, (hipStream_t)stream, dyn_args(s, v), ground_dev, ball_dev, pairs_dev);
}
// ---- query states: include/bez_sim.h "Query states"
static bool owns(const BezSim* s, const BezQueryState* q) { return std::find(s->queries.begin(), s->queries.end(), q) != s->queries.end(); }
// the shared front of every call on a query state: both handles, and the state is one of this sim's
#define QS_TRY(s, q, name)                                                                            \
  do {                                                                                                \
    if (!(s)) return fail((s), -1, name ": sim is null");                                             \
    if (!(q)) return fail((s), -1, name ": the query state is null");                                 \
    if (!owns((s), (q))) return fail((s), -1, name ": the query state belongs to another sim");       \
  } while (0)

int bez_query_state_create(BezSim* s, int32_t rows, BezQueryState** out) {
  if (!s) return fail(s, -1, "bez_query_state_create: sim is null");
  if (!out) return fail(s, -1, "bez_query_state_create: out is null");
  *out = nullptr;
  if (rows <= 0) return fail(s, -1, "bez_query_state_create: rows must be > 0");
  BezQueryState* q = new (std::nothrow) BezQueryState();
  if (!q) return fail(s, -4, "out of host memory");
  q->sim = s; q->rows = rows;
  s->queries.push_back(q);
  (void)hipSetDevice(s->device);
  int rc = dev_alloc_zeroed(s, &q->state, (size_t)rows * QS_FIELDS * sizeof(float));
  for (int p = 0; p < QS_PARAMS && !rc; ++p) rc = dev_alloc_zeroed(s, &q->param[p], (size_t)rows * QS_PARAM_WIDTH[p] * sizeof(float));
  if (rc) { const std::string why = s->err; bez_query_state_destroy(s, q); s->err = why; return rc; }
  *out = q;
  return 0;
}
int bez_query_state_destroy(BezSim* s, BezQueryState* q) {
  QS_TRY(s, q, "bez_query_state_destroy");
  if (s->bound == q) return fail(s, -1, "bez_query_state_destroy: the query state is bound (unbind it first: bez_query_state_bind(sim, NULL))");
  (void)hipSetDevice(s->device);
  float** slots[] = {&q->state, &q->param[0], &q->param[1], &q->param[2], &q->param[3], &q->rigid_body, &q->jacobian, &q->mass_matrix};
  for (float** slot : slots) if (*slot) dev_free(s, slot);   // (hipFree waits for the work that may still read the buffer)
  s->queries.erase(std::remove(s->queries.begin(), s->queries.end(), q), s->queries.end());
  delete q;
  return 0;
}
}  // extern "C"
// what set and capture share: the destination, the sim's parameter rows, the config's constants; then the launch over the tiles
static QsFill fill_args(const BezSim* s, BezQueryState* q, const int32_t* ids) {
  QsFill A = {};
  A.st = q->state; A.rows = q->rows; A.n = s->n; A.ids = ids;
  for (int p = 0; p < QS_PARAMS; ++p) { A.param[p] = q->param[p]; A.src_param[p] = s->dr[QS_PARAM_ID[p]]; }
  for (int k = 0; k < 7; ++k) A.ball_rest[k] = s->cfg.ball_init[k];
  for (int k = 0; k < 3; ++k) A.g[k] = s->cfg.gravity[k];
  return A;
}
template <bool CAPTURE>
static int launch_fill(BezSim* s, const QsFill& A, hipStream_t stream) {
  return launch_checked<QS_THREADS>(s, "query_state_fill_kernel launch", query_state_fill_kernel<CAPTURE>,
                                    (size_t)((A.rows + QS_TILE - 1) / QS_TILE) * QS_THREADS, stream, A);
}
extern "C" {
int bez_query_state_set(BezSim* s, BezQueryState* q, const float* root_dev, const float* dof_dev, const float* ball_dev, const int32_t* env_ids_dev,
                        void* stream) {
  QS_TRY(s, q, "bez_query_state_set");
  if (!root_dev || !dof_dev) return fail(s, -1, "bez_query_state_set: root_dev or dof_dev is null");
  if (ball_dev && !s->has_ball) return fail(s, -1, "bez_query_state_set: ball_dev given, but this task has no ball");
  QsFill A = fill_args(s, q, env_ids_dev);
  A.root = root_dev; A.dof = dof_dev; A.ball = ball_dev;
  // without ids every row is nominal: the kernels see null parameter pointers; with ids, the rows the sim has
  for (int p = 0; p < QS_PARAMS; ++p) q->shown[p] = env_ids_dev && A.src_param[p];
  return launch_fill<false>(s, A, (hipStream_t)stream);
}
int bez_query_state_capture(BezSim* s, BezQueryState* q, const int32_t* env_ids_dev, void* stream) {
  QS_TRY(s, q, "bez_query_state_capture");
  if (!env_ids_dev && q->rows != s->n) return fail(s, -1, "bez_query_state_capture: env_ids_dev is null (row i <- env i), which needs rows == num_envs");
  QsFill A = fill_args(s, q, env_ids_dev);
  A.src_st = s->state;
  for (int p = 0; p < QS_PARAMS; ++p) q->shown[p] = A.src_param[p] != nullptr;
  return launch_fill<true>(s, A, (hipStream_t)stream);
}
int bez_query_state_bind(BezSim* s, BezQueryState* q) {
  if (!s) return fail(s, -1, "bez_query_state_bind: sim is null");
  if (q && !owns(s, q)) return fail(s, -1, "bez_query_state_bind: the query state belongs to another sim");
  s->bound = q;
  return 0;
}
int bez_query_state_tensor(BezSim* s, BezQueryState* q, int which, void** dev_ptr, int64_t shape[3], int* ndim, int* dtype) {
  QS_TRY(s, q, "bez_query_state_tensor");
  if (!dev_ptr || !shape || !ndim || !dtype) return fail(s, -1, "bez_query_state_tensor: null argument");
  float** slot = nullptr;
  switch (which) {
    case BEZ_QUERY_RIGID_BODY_STATE: slot = &q->rigid_body; shape[0] = (int64_t)q->rows * s->nbe; shape[1] = 13; shape[2] = 0; *ndim = 2; break;
    case BEZ_QUERY_JACOBIAN: slot = &q->jacobian; shape[0] = (int64_t)q->rows * s->nb; shape[1] = 6; shape[2] = 6 + BEZ_ND; *ndim = 3; break;
    case BEZ_QUERY_MASS_MATRIX: slot = &q->mass_matrix; shape[0] = q->rows; shape[1] = shape[2] = 6 + BEZ_ND; *ndim = 3; break;
    default: return fail(s, -1, "bez_query_state_tensor: unknown tensor id");
  }
  if (!*slot) {   // the acquisition: the one place that allocates (and, through hipMemset, waits)
    (void)hipSetDevice(s->device);
    RC_TRY(dev_alloc_zeroed(s, slot, (size_t)(shape[0] * shape[1] * (shape[2] ? shape[2] : 1)) * sizeof(float)));
  }
  *dev_ptr = *slot; *dtype = BEZ_DTYPE_F32;
  return 0;
}
int bez_query_state_refresh(BezSim* s, BezQueryState* q, uint32_t which_mask, void* stream) {
  QS_TRY(s, q, "bez_query_state_refresh");
  if (which_mask == 0u || (which_mask >> BEZ_QUERY_TENSOR_COUNT)) return fail(s, -1, "bez_query_state_refresh: which_mask must be a non-empty set of (1u << BezQueryTensor) bits");
  const bool rb = which_mask & (1u << BEZ_QUERY_RIGID_BODY_STATE), jac = which_mask & (1u << BEZ_QUERY_JACOBIAN), mm = which_mask & (1u << BEZ_QUERY_MASS_MATRIX);
  if ((rb && !q->rigid_body) || (jac && !q->jacobian) || (mm && !q->mass_matrix))
    return fail(s, -1, "bez_query_state_refresh: a requested tensor was never acquired (bez_query_state_tensor allocates it)");
  const StateView v = view_of(q);
  if (rb) RC_TRY(LAUNCH_VIEW(s, v, refresh_rigid_body_kernel, 64, 64, (hipStream_t)stream, v.st, q->rigid_body, v.n, (int)v.has_ball, s->cfg.flags));
  if (jac || mm)
    RC_TRY(LAUNCH_VIEW(s, v, refresh_dynamics_kernel, DYN_TILE, DYN_THREADS, (hipStream_t)stream, dyn_args(s, v), jac ? q->jacobian : nullptr,
                       mm ? q->mass_matrix : nullptr));
  return 0;
}

int bez_sim_set_obs_calls(BezSim* s, int64_t calls) { if (!s) return -1; s->obs_calls = calls; return 0; }

int bez_sim_pre_physics(BezSim* s, const float* actions_dev, void* stream) {
  if (!s || !actions_dev) return fail(s, -1, "bez_sim_pre_physics: bad argument");
  return launch_step<true, false, false>(s, actions_dev, (hipStream_t)stream);
}
int bez_sim_simulate(BezSim* s, void* stream) {
  if (!s) return -1;
  return launch_step<false, true, false>(s, nullptr, (hipStream_t)stream);
}
int bez_sim_post_physics(BezSim* s, void* stream) {
  if (!s) return -1;
  return launch_step<false, false, true>(s, nullptr, (hipStream_t)stream);
}
/* test hook: compute_observations + compute_reward only (no timeout/progress/reset bookkeeping) */
int bez_sim_observe_reward(BezSim* s, void* stream) {
  if (!s) return -1;
  return launch_step<false, false, true>(s, nullptr, (hipStream_t)stream, /*obs_only=*/true);
}
/* (N,2) per-env goal of bez_walk (test hook; walk_env.py:143,570-575) */
int bez_sim_set_goal_tensor(BezSim* s, const float* goal_dev, void* stream) {
  return scatter_rows(s, BEZ_TENSOR_GOAL, goal_dev, stream, "set_goal_tensor: bad argument");
}
int bez_sim_step(BezSim* s, const float* actions_dev, void* stream) {
  if (!s || !actions_dev) return fail(s, -1, "bez_sim_step: bad argument");
  return launch_step<true, true, true>(s, actions_dev, (hipStream_t)stream);
}
int bez_sim_step_many(BezSim* s, const float* actions_dev, int32_t n_steps, void* stream) {
  if (!s || !actions_dev || n_steps < 0) return fail(s, -1, "bez_sim_step_many: bad argument");
  for (int32_t t = 0; t < n_steps; ++t) {
    int rc = launch_step<true, true, true>(s, actions_dev + (size_t)t * s->n * BEZ_ND, (hipStream_t)stream);
    if (rc) return rc;
  }
  return 0;
}
int bez_sim_time_steps(BezSim* s, const float* actions_dev, int32_t n_steps, void* stream_, float* avg_ms) {
  if (!s || !actions_dev || n_steps <= 0 || !avg_ms) return fail(s, -1, "bez_sim_time_steps: bad argument");
  hipStream_t stream = (hipStream_t)stream_;
  HIP_TRY(s, hipEventRecord(s->ev0, stream));
  int rc = bez_sim_step_many(s, actions_dev, n_steps, stream_);
  if (rc) return rc;
  HIP_TRY(s, hipEventRecord(s->ev1, stream));
  HIP_TRY(s, hipEventSynchronize(s->ev1));
  float ms = 0.f;
  HIP_TRY(s, hipEventElapsedTime(&ms, s->ev0, s->ev1));
  *avg_ms = ms / (float)n_steps;
  return 0;
}

int bez_sim_reset_indexed(BezSim* s, const int32_t* env_ids_dev, int32_t count, void* stream) {
  if (!s || (!env_ids_dev && count > 0) || count < 0) return fail(s, -1, "bez_sim_reset_indexed: bad argument");
  if (count == 0) return 0;
  Params P = make_params(s, nullptr);
  goal_draw(s->cfg.seed, s->reset_calls++, 1, P.goal_draw);
  return LAUNCH(s, reset_kernel, (size_t)count, (hipStream_t)stream, P, env_ids_dev, count);
}

// (N, width) of every BezEnvParam (abi.PARAM_WIDTH is the Python mirror)
static constexpr int PARAM_WIDTH[BEZ_PARAM_COUNT] = {1, BEZ_ND, BEZ_ND, BEZ_NL, 3, BEZ_ND, BEZ_ND};

int bez_sim_set_env_params(BezSim* s, int param, const float* values_dev, void* stream) {
  if (!s || param < 0 || param >= BEZ_PARAM_COUNT) return fail(s, -1, "bez_sim_set_env_params: bad argument");
  const bool packed = param == BEZ_PARAM_KP_SCALE || param == BEZ_PARAM_KD_SCALE || param == BEZ_PARAM_DOF_LOWER || param == BEZ_PARAM_DOF_UPPER;
  if (param == BEZ_PARAM_GRAVITY) s->gravity_uniform = false;   // rows written from outside may differ from env to env
  if (!values_dev) {
    if (s->dr[param]) { HIP_TRY(s, hipStreamSynchronize((hipStream_t)stream)); dev_free(s, &s->dr[param]); }
  } else {
    const size_t bytes = (size_t)s->n * PARAM_WIDTH[param] * sizeof(float);
    if (!s->dr[param]) RC_TRY(dev_alloc_zeroed(s, &s->dr[param], bytes, (hipStream_t)stream));
    HIP_TRY(s, hipMemcpyAsync(s->dr[param], values_dev, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  }
  if (packed && repack_dr(s, (hipStream_t)stream)) return fail(s, -2, "bez_sim_set_env_params: repack");
  return 0;
}

struct ParamRow { float v[BEZ_NL]; };   // the widest row, passed to the kernel by value
__global__ void fill_rows_kernel(float* out, ParamRow row, int width, size_t total) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) out[i] = row.v[i % width];
}
// the default rows of a parameter (what the step uses while the parameter is not set): only enqueues work on `stream`
static int fill_default_params(BezSim* s, int param, float* out_dev, hipStream_t stream) {
  const int width = PARAM_WIDTH[param];
  ParamRow row = {};
  for (int k = 0; k < width; ++k) {
    switch (param) {
      case BEZ_PARAM_FRICTION: row.v[k] = s->cfg.plane_friction; break;
      case BEZ_PARAM_GRAVITY: row.v[k] = s->cfg.gravity[k]; break;
      case BEZ_PARAM_DOF_LOWER: row.v[k] = (float)BEZ_DOF_LOWER[k]; break;
      case BEZ_PARAM_DOF_UPPER: row.v[k] = (float)BEZ_DOF_UPPER[k]; break;
      default: row.v[k] = 1.0f; break;
    }
  }
  return LAUNCH(s, fill_rows_kernel, (size_t)s->n * width, stream, out_dev, row, width, (size_t)s->n * width);
}

int bez_sim_get_env_params(BezSim* s, int param, float* out_dev, void* stream) {
  if (!s || !out_dev || param < 0 || param >= BEZ_PARAM_COUNT) return fail(s, -1, "bez_sim_get_env_params: bad argument");
  if (!s->dr[param]) return fill_default_params(s, param, out_dev, (hipStream_t)stream);
  HIP_TRY(s, hipMemcpyAsync(out_dev, s->dr[param], (size_t)s->n * PARAM_WIDTH[param] * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

int bez_sim_add_dr_noise(BezSim* s, const float* x_dev, float* y_dev, int64_t n, int32_t which, void* stream_) {
  if (!s || !x_dev || !y_dev || n < 0 || which < 0 || which > 1) return fail(s, -1, "bez_sim_add_dr_noise: bad argument");
  if (n == 0) return 0;
  if (which == 0 && x_dev == s->obs && y_dev == s->obs && s->obs_noise_applied) return 0;   // the step kernel already added it (BEZ_FLAG_OBS_NOISE_IN_STEP)
  const long long quads = (n + 3) / 4;
  return LAUNCH(s, dr_noise_kernel, (size_t)quads, (hipStream_t)stream_, x_dev, y_dev, (long long)n, s->dr_state, s->dr_snap, (int)which, s->cfg.seed, s->cfg.env_id_offset);
}

/* The randomisation kernel of the COMING control step, now, on `stream` (the step then skips its own): the caller may overlap it with
 * whatever else precedes that step (a policy forward pass), on another stream, as long as that stream is joined before the step.
 * Needs: the previous step's post-physics has finished on a stream `stream` is ordered behind. */
int bez_sim_dr_prelaunch(BezSim* s, void* stream_) {
  if (!s) return -1;
  if (!s->dr_on) return 0;
  if (s->dr_prelaunched) return fail(s, -1, "bez_sim_dr_prelaunch: already launched for the coming step");
  launch_dr(s, false, (hipStream_t)stream_);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(s, -2, "dr_kernel launch", e);
  s->dr_prelaunched = true;
  return 0;
}
int bez_sim_dr_step_args(BezSim* s, void* blob, int32_t blob_bytes) {
  if (!s || !blob || blob_bytes < (int32_t)sizeof(DrArgs)) return fail(s, -1, "bez_sim_dr_step_args: bad argument");
  if (!s->dr_on) return 0;
  if (s->dr_prelaunched) return fail(s, -1, "bez_sim_dr_step_args: the coming step's randomisation was already handed out");
  std::memset(blob, 0, (size_t)blob_bytes);
  const DrArgs A = make_dr_args(s, false);
  std::memcpy(blob, &A, sizeof(A));
  s->dr_prelaunched = true;
  return (int)sizeof(DrArgs);
}
int bez_sim_dr_cancel(BezSim* s) {
  if (!s) return -1;
  s->dr_prelaunched = false;
  return 0;
}
/* Where a consumer that adds the action noise ITSELF (vec_task.py:586-592; e.g. bez_ppo_policy_rollout_step's epilogue) finds its
 * parameters: a device struct {float mean, std; uint32 frame_lo, frame_hi} kept by the step kernels, and the Philox key parts.  The
 * noise of element i of the flat (N, 18) action tensor is mean + std * z with z = word (i & 3) of dr-noise quad (i >> 2) for which = 1
 * -- the same bits bez_sim_add_dr_noise(which = 1) adds.  Returns 1 if an action noise is configured, 0 if not. */
int bez_sim_action_noise_source(BezSim* s, const void** snap_dev, uint64_t* seed, int64_t* env_id_offset) {
  if (!s || !snap_dev || !seed || !env_id_offset) return -1;
  *snap_dev = s->dr_snap; *seed = s->cfg.seed; *env_id_offset = s->cfg.env_id_offset;
  return (s->dr_on && s->drc.actions.enabled) ? 1 : 0;
}

int bez_sim_set_randomization(BezSim* s, const BezDrConfig* dr, void* stream_) {
  if (!s) return -1;
  hipStream_t stream = (hipStream_t)stream_;
  s->dr_prelaunched = false;   // a hand-out made under the previous configuration is void
  if (!dr) { s->dr_on = false; return 0; }
  if (dr->frequency < 1) return fail(s, -1, "bez_sim_set_randomization: frequency must be >= 1");
  s->drc = *dr;
  // the per-env arrays the kernel writes: created with the defaults (bez_sim_get_env_params fills them) where not set yet
  const struct { int param; int on; } need[] = {{BEZ_PARAM_FRICTION, dr->friction.enabled}, {BEZ_PARAM_KP_SCALE, dr->stiffness.enabled},
                                                {BEZ_PARAM_KD_SCALE, dr->damping.enabled}, {BEZ_PARAM_DOF_LOWER, dr->lower.enabled},
                                                {BEZ_PARAM_DOF_UPPER, dr->upper.enabled}, {BEZ_PARAM_GRAVITY, dr->gravity.enabled}};
  for (const auto& nd : need) {
    if (!nd.on || s->dr[nd.param]) continue;
    RC_TRY(dev_alloc_zeroed(s, &s->dr[nd.param], (size_t)s->n * PARAM_WIDTH[nd.param] * sizeof(float), stream));
    if (int rc = fill_default_params(s, nd.param, s->dr[nd.param], stream)) { dev_free(s, &s->dr[nd.param]); return rc; }
  }
  HIP_TRY(s, hipMemsetAsync(s->dr_state, 0, sizeof(DrState), stream));
  s->dr_on = true;
  if (repack_dr(s, stream)) return fail(s, -2, "bez_sim_set_randomization: repack");   // (the randomisation kernel keeps it current from here on)
  // gravity rows: from now on written by the randomisation kernel only, one vector for the whole sim.  (Rows that were set per env
  // BEFORE stay as they are until the first gravity redraw: only then are they known to be uniform -- the kernel says when.)
  s->gravity_uniform = false;
  launch_dr(s, true, stream);   // first_randomization (vec_task.py:521-523): every env, frame 0
  if (dr->gravity.enabled) s->gravity_uniform = true;   // the first randomisation redraws gravity for every env (A.first => nonenv)
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(s, -2, "dr_kernel launch", e);
  return 0;
}

#ifdef BEZ_WS_STAMPS
/* diagnostic build only: run one fused step and return the 8 x 32 s_memtime stamps (roles x phase boundaries) of workgroup 0 */
int bez_sim_debug_stamps(BezSim* s, const float* actions_dev, unsigned long long* out_host) {
  if (!s->stamps) RC_TRY(dev_alloc_zeroed(s, &s->stamps, 256 * sizeof(unsigned long long)));
  HIP_TRY(s, hipMemset(s->stamps, 0, 256 * sizeof(unsigned long long)));
  RC_TRY(bez_sim_step(s, actions_dev, nullptr));
  HIP_TRY(s, hipDeviceSynchronize());
  HIP_TRY(s, hipMemcpy(out_host, s->stamps, 256 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return 0;
}
#endif

/* Measurement utility (tools/pmc_calibrate.py): known-size dword-per-lane read / write kernels to calibrate the
 * FETCH_SIZE / WRITE_SIZE counters for this library's access shape (MI355X_MICROARCH.md: only 16 B/lane is calibrated). */
int bez_sim_calibrate(void* buf_dev, uint64_t n_floats, int32_t write, void* stream) {
  if (!buf_dev || n_floats == 0) return -1;
  if (write) hipLaunchKernelGGL(calib_write_kernel, dim3(2048), dim3(256), 0, (hipStream_t)stream, (float*)buf_dev, (size_t)n_floats);
  else hipLaunchKernelGGL(calib_read_kernel, dim3(2048), dim3(256), 0, (hipStream_t)stream, (const float*)buf_dev, (float*)buf_dev, (size_t)n_floats);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int bez_sim_health(BezSim* s, uint64_t* bits, int32_t clear, void* stream_) {
  if (!s || !bits) return fail(s, -1, "bez_sim_health: null argument");
  hipStream_t stream = (hipStream_t)stream_;
  unsigned long long h = 0;
  HIP_TRY(s, hipMemcpyAsync(&h, s->health, sizeof(h), hipMemcpyDeviceToHost, stream));
  if (clear) HIP_TRY(s, hipMemsetAsync(s->health, 0, sizeof(h), stream));
  HIP_TRY(s, hipStreamSynchronize(stream));
  *bits = (uint64_t)h;
  return 0;
}

int bez_sim_apply_body_forces(BezSim* s, const float* forces_dev, const float* torques_dev, const float* positions_dev, int32_t space, void* stream_) {
  if (!s) return -1;
  if (space != BEZ_SPACE_ENV && space != BEZ_SPACE_LOCAL) return fail(s, -1, "bez_sim_apply_body_forces: space must be BEZ_SPACE_ENV or BEZ_SPACE_LOCAL");
  hipStream_t stream = (hipStream_t)stream_;
  if (!s->ext) {   // first call: the pending buffer (zeroed in stream order), and the switch to the EXT kernels for the rest of the sim's life
    RC_TRY(dev_alloc_zeroed(s, &s->ext, (size_t)EXT_WORDS * s->n * sizeof(float), stream));
    s->ext_on = true;
  }
  if (!forces_dev && !torques_dev) return 0;
  return LAUNCH_ASSET(s, ext_prepare_kernel, 64, 64, stream, s->state, s->ext, forces_dev, torques_dev, positions_dev, (int)space, s->n, (int)s->has_ball, s->cfg.flags);
}

int bez_sim_seed(BezSim* s, uint64_t seed) { if (!s) return -1; s->cfg.seed = seed; s->dr_prelaunched = false; return 0; }

}  // extern "C"

// =============================================================================================== env snapshots (include/bez_sim.h)
// The inventory of "what is an env": one SNAP_TABLE row per per-env buffer of BezSim that a snapshot keeps (DESIGN.md 4.3p lists every
// buffer, also the derived ones and the ones left alone).  A new per-env buffer that decides how an env continues is one row here, one
// name in abi.SNAPSHOT_SECTIONS and BEZ_SNAPSHOT_SECTIONS + 1; the rewind tests fail without it.
namespace {
enum : int { SNAP_SEC_PARAM0 = 12, SNAP_SEC_DF = SNAP_SEC_PARAM0 + BEZ_PARAM_COUNT };
static_assert(SNAP_SEC_DF + 1 == BEZ_SNAPSHOT_SECTIONS && BEZ_SNAPSHOT_SECTIONS <= SNAP_MAX_SECTIONS, "the sections of a snapshot");
struct SnapRow { int kind; int width; /* < 0: by sim, below */ void* (*env)(const BezSim*); };
enum : int { W_OBS = -1, W_PARAM = -2, W_DF = -3 };
#define ENV(expr) [](const BezSim* s) -> void* { return (void*)(expr); }
const SnapRow SNAP_TABLE[BEZ_SNAPSHOT_SECTIONS] = {
    {SNAP_COL, F_COUNT, ENV(s->state)},
    {SNAP_ROW, W_OBS, ENV(s->obs)},
    {SNAP_COL, 1, ENV(s->rew)},
    {SNAP_COL64, 2, ENV(s->reset)},
    {SNAP_COL64, 2, ENV(s->progress)},
    {SNAP_COL64, 2, ENV(s->timeout)},
    {SNAP_COL, 1, ENV(s->episode)},
    {SNAP_COL64, 2, ENV(s->randomize)},
    {SNAP_COL64, 2, ENV(s->nonfinite)},
    {SNAP_COL64, 2 * BEZ_END_CAUSES, ENV(s->episode_stats)},                                                       // end counts (8, N) i64
    {SNAP_COL, BEZ_END_CAUSES, ENV(s->episode_stats + (size_t)BEZ_END_CAUSES * s->n)},                             // reward terms (8, N) f32
    {SNAP_COL, 1, ENV((float*)(s->episode_stats + (size_t)BEZ_END_CAUSES * s->n) + (size_t)BEZ_END_CAUSES * s->n)},   // end bits (N) i32
    {SNAP_ROW, W_PARAM, ENV(s->dr[0])}, {SNAP_ROW, W_PARAM, ENV(s->dr[1])}, {SNAP_ROW, W_PARAM, ENV(s->dr[2])}, {SNAP_ROW, W_PARAM, ENV(s->dr[3])},
    {SNAP_ROW, W_PARAM, ENV(s->dr[4])}, {SNAP_ROW, W_PARAM, ENV(s->dr[5])}, {SNAP_ROW, W_PARAM, ENV(s->dr[6])},
    {SNAP_COL, W_DF, ENV(s->df_raw)},                                                                               // [substep][3][dof][env]
};
#undef ENV
int snap_width(const BezSim* s, int sec) {
  const int w = SNAP_TABLE[sec].width;
  return w == W_OBS ? s->nobs : w == W_PARAM ? PARAM_WIDTH[sec - SNAP_SEC_PARAM0] : w == W_DF ? (s->df_raw ? s->cfg.substeps * 3 * BEZ_ND : 0) : w;
}
// the sim-global device words, in the order the snapshot keeps them
constexpr int SNAP_GLOBAL_WORDS[SNAP_GLOBALS] = {2, (int)(sizeof(DrState) / 4), (int)(sizeof(DrSnap) / 4), 2};
static_assert(SNAP_GLOBAL_WORDS[0] + SNAP_GLOBAL_WORDS[1] + SNAP_GLOBAL_WORDS[2] + SNAP_GLOBAL_WORDS[3] == BEZ_SNAPSHOT_GLOBAL_WORDS &&
              sizeof(DrState) % 4 == 0 && sizeof(DrSnap) % 4 == 0, "the global device words of a snapshot");
}  // namespace

struct BezSnapshot {
  BezSim* sim = nullptr;
  int rows = 0;
  uint32_t* data = nullptr;                      // device: `cols` columns of `rows` words, then BEZ_SNAPSHOT_GLOBAL_WORDS
  int width[BEZ_SNAPSHOT_SECTIONS] = {};
  uint32_t off[BEZ_SNAPSHOT_SECTIONS] = {}, cols = 0;
  uint32_t present = 0;                          // bit per section: what the last save found in its sim (0: nothing was saved yet)
  int64_t obs_calls = 0;                         // the host part of the global block, as the last save found it
  uint64_t post_calls = 0, reset_calls = 0;
  uint32_t gravity_uniform = 0, obs_noise_applied = 0;
  int grid_y = 0;                                // BEZ_SNAPSHOT_GRID_Y at creation, a measurement knob (tools/snapshot_times.py): workgroups over the
                                                 // chunks of columns per tile of entries; 0: one per chunk (DESIGN.md 4.3p has both timings)
};

namespace {
void forget_snapshot(const BezSnapshot* p) {
  std::lock_guard<std::mutex> lock(g_snapshots_mutex);
  g_snapshots.erase(std::remove(g_snapshots.begin(), g_snapshots.end(), p), g_snapshots.end());
}
bool snapshot_alive(const BezSnapshot* p) {
  std::lock_guard<std::mutex> lock(g_snapshots_mutex);
  return std::find(g_snapshots.begin(), g_snapshots.end(), p) != g_snapshots.end();
}
// the shared front of the calls on a snapshot
#define SNAP_TRY(s, p, name, own)                                                                                       \
  do {                                                                                                                  \
    if (!(s)) return fail((s), -1, name ": sim is null");                                                               \
    if (!(p)) return fail((s), -1, name ": the snapshot is null");                                                      \
    if (!snapshot_alive(p)) return fail((s), -1, name ": the snapshot is not alive (destroyed, or never created)");      \
    if ((own) && (p)->sim != (s)) return fail((s), -1, name ": the snapshot belongs to another sim");                    \
  } while (0)
size_t snap_words(const BezSnapshot* p) { return (size_t)p->cols * p->rows + BEZ_SNAPSHOT_GLOBAL_WORDS; }
uint32_t snap_asset(const BezSim* s) { return s->cfg.flags & (BEZ_FLAG_CLEATS | BEZ_FLAG_BOX_ASSET); }

void snap_header(const BezSim* s, const BezSnapshot* p, uint32_t h[BEZ_SNAPSHOT_HEADER_WORDS]) {
  std::memset(h, 0, BEZ_SNAPSHOT_HEADER_WORDS * sizeof(uint32_t));
  h[0] = BEZ_SNAPSHOT_MAGIC; h[1] = BEZ_SNAPSHOT_LAYOUT; h[2] = (uint32_t)p->rows; h[3] = BEZ_SNAPSHOT_SECTIONS; h[4] = p->present; h[5] = p->cols;
  h[6] = BEZ_SNAPSHOT_GLOBAL_WORDS;
  for (int k = 0; k < BEZ_SNAPSHOT_SECTIONS; ++k) h[8 + k] = (uint32_t)p->width[k];
  uint32_t* g = h + 8 + BEZ_SNAPSHOT_SECTIONS;
  g[0] = (uint32_t)p->obs_calls; g[1] = (uint32_t)((uint64_t)p->obs_calls >> 32); g[2] = (uint32_t)p->post_calls; g[3] = (uint32_t)(p->post_calls >> 32);
  g[4] = (uint32_t)p->reset_calls; g[5] = (uint32_t)(p->reset_calls >> 32); g[6] = p->gravity_uniform; g[7] = p->obs_noise_applied;
  g[8] = (uint32_t)s->cfg.task; g[9] = snap_asset(s); g[10] = s->has_ball ? 1u : 0u; g[11] = (uint32_t)s->nobs;
}
static_assert(8 + BEZ_SNAPSHOT_SECTIONS + 12 == BEZ_SNAPSHOT_HEADER_WORDS, "the header of a snapshot blob");

// The launch of a save (SAVE) or a restore on sim `s`: the sections by `mode`, in chunks of columns over the second grid dimension
template <bool SAVE>
int launch_snapshot(BezSim* s, const BezSnapshot* p, const int mode[BEZ_SNAPSHOT_SECTIONS], const int32_t* env_ids, const int32_t* row_ids, int count,
                    bool globals, hipStream_t stream) {
  SnapArgs A = {};
  A.snap = p->data; A.rows = p->rows; A.n = s->n; A.env_ids = env_ids; A.row_ids = row_ids; A.count = count;
  A.glob_snap = p->data + (size_t)p->cols * p->rows;
  uint32_t* glob[SNAP_GLOBALS] = {(uint32_t*)s->post_calls_dev, (uint32_t*)s->dr_state, (uint32_t*)s->dr_snap, (uint32_t*)s->goal_draw_dev};
  for (int g = 0; g < SNAP_GLOBALS; ++g) { A.glob[g] = globals ? glob[g] : nullptr; A.glob_words[g] = SNAP_GLOBAL_WORDS[g]; }
  for (int k = 0; k < BEZ_PARAM_COUNT; ++k)
    for (int j = 0; j < PARAM_WIDTH[k]; ++j)
      A.dflt[k][j] = k == BEZ_PARAM_FRICTION ? s->cfg.plane_friction : k == BEZ_PARAM_GRAVITY ? s->cfg.gravity[j] : k == BEZ_PARAM_DOF_LOWER ? (float)BEZ_DOF_LOWER[j]
                     : k == BEZ_PARAM_DOF_UPPER ? (float)BEZ_DOF_UPPER[j] : 1.0f;   // (the rows of fill_default_params)
  for (int chunk_words = SNAP_CHUNK;; chunk_words *= 2) {   // (a long actuator record: wider chunks until the table holds them)
    int nc = 0;
    for (int k = 0; k < BEZ_SNAPSHOT_SECTIONS && nc <= SNAP_MAX_CHUNKS; ++k) {
      SnapSection& S = A.sec[k];
      S.env = (uint32_t*)SNAP_TABLE[k].env(s); S.off = p->off[k]; S.width = p->width[k]; S.kind = SNAP_TABLE[k].kind; S.mode = mode[k];
      S.dflt = k >= SNAP_SEC_PARAM0 && k < SNAP_SEC_DF ? k - SNAP_SEC_PARAM0 : 0;
      if (S.mode == SNAP_SKIP || S.width == 0) continue;
      const int step = S.kind == SNAP_ROW ? S.width : chunk_words;
      for (int w0 = 0; w0 < S.width; w0 += step, ++nc)
        if (nc < SNAP_MAX_CHUNKS) A.chunk[nc] = {(int16_t)k, (int16_t)w0, (int16_t)std::min(step, S.width - w0), 0};
    }
    if (nc <= SNAP_MAX_CHUNKS) { A.nchunks = nc; break; }
  }
  const dim3 grid((unsigned)std::max(1, (count + SNAP_TILE - 1) / SNAP_TILE), (unsigned)std::max(1, p->grid_y > 0 ? std::min(p->grid_y, A.nchunks) : A.nchunks));
  hipLaunchKernelGGL(snapshot_copy_kernel<SAVE>, grid, dim3(SNAP_THREADS), 0, stream, A);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(s, -2, "snapshot_copy_kernel launch", e);
}
}  // namespace

static void forget_snapshots(BezSim* s) {   // bez_sim_destroy: their buffers went with the sim's
  for (BezSnapshot* p : s->snapshots) { forget_snapshot(p); delete p; }
  s->snapshots.clear();
}

extern "C" {
int bez_snapshot_create(BezSim* s, int32_t rows, BezSnapshot** out) {
  if (!s) return fail(s, -1, "bez_snapshot_create: sim is null");
  if (!out) return fail(s, -1, "bez_snapshot_create: out is null");
  *out = nullptr;
  if (rows < 1) return fail(s, -1, "bez_snapshot_create: rows must be >= 1");
  BezSnapshot* p = new (std::nothrow) BezSnapshot();
  if (!p) return fail(s, -4, "out of host memory");
  p->sim = s; p->rows = rows;
  if (const char* v = std::getenv("BEZ_SNAPSHOT_GRID_Y")) p->grid_y = std::atoi(v);
  for (int k = 0; k < BEZ_SNAPSHOT_SECTIONS; ++k) { p->width[k] = snap_width(s, k); p->off[k] = p->cols; p->cols += (uint32_t)p->width[k]; }
  (void)hipSetDevice(s->device);
  if (int rc = dev_alloc_zeroed(s, &p->data, snap_words(p) * sizeof(uint32_t))) { delete p; return rc; }
  s->snapshots.push_back(p);
  { std::lock_guard<std::mutex> lock(g_snapshots_mutex); g_snapshots.push_back(p); }
  *out = p;
  return 0;
}
int bez_snapshot_destroy(BezSim* s, BezSnapshot* p) {
  SNAP_TRY(s, p, "bez_snapshot_destroy", true);
  (void)hipSetDevice(s->device);
  dev_free(s, &p->data);   // (hipFree waits for the work that may still read the buffer)
  s->snapshots.erase(std::remove(s->snapshots.begin(), s->snapshots.end(), p), s->snapshots.end());
  forget_snapshot(p);
  delete p;
  return 0;
}
int bez_snapshot_save(BezSim* s, BezSnapshot* p, const int32_t* env_ids_dev, void* stream) {
  SNAP_TRY(s, p, "bez_snapshot_save", true);
  int mode[BEZ_SNAPSHOT_SECTIONS];
  uint32_t present = 0;
  for (int k = 0; k < BEZ_SNAPSHOT_SECTIONS; ++k) {
    const bool has = SNAP_TABLE[k].env(s) != nullptr && p->width[k] > 0 && snap_width(s, k) == p->width[k];
    mode[k] = has ? SNAP_COPY : SNAP_SKIP;
    if (has) present |= 1u << k;
  }
  RC_TRY(launch_snapshot<true>(s, p, mode, env_ids_dev, nullptr, p->rows, true, (hipStream_t)stream));
  p->present = present;
  p->obs_calls = s->obs_calls; p->post_calls = s->post_calls; p->reset_calls = s->reset_calls;
  p->gravity_uniform = s->gravity_uniform ? 1u : 0u; p->obs_noise_applied = s->obs_noise_applied ? 1u : 0u;
  return 0;
}
int bez_snapshot_restore(BezSim* d, const BezSnapshot* p, const int32_t* env_ids_dev, const int32_t* row_ids_dev, int32_t count, uint32_t what,
                         void* stream_) {
  SNAP_TRY(d, p, "bez_snapshot_restore", false);
  hipStream_t stream = (hipStream_t)stream_;
  if (count < 0) return fail(d, -1, "bez_snapshot_restore: count must be >= 0");
  if (!row_ids_dev && count > p->rows) return fail(d, -1, "bez_snapshot_restore: count exceeds the snapshot's rows (row_ids_dev is null: row i)");
  if (!(what & BEZ_SNAPSHOT_ENVS) || (what & ~(uint32_t)(BEZ_SNAPSHOT_ENVS | BEZ_SNAPSHOT_GLOBALS)))
    return fail(d, -1, "bez_snapshot_restore: what must be BEZ_SNAPSHOT_ENVS or BEZ_SNAPSHOT_ENVS | BEZ_SNAPSHOT_GLOBALS");
  if (!p->present) return fail(d, -1, "bez_snapshot_restore: nothing was saved into the snapshot yet");
  const BezSim* o = p->sim;
  if (d != o) {
    if (d->device != o->device) return fail(d, -1, "bez_snapshot_restore: incompatible destination: another device");
    if (d->cfg.task != o->cfg.task) return fail(d, -1, "bez_snapshot_restore: incompatible destination: another task");
    if (snap_asset(d) != snap_asset(o)) return fail(d, -1, "bez_snapshot_restore: incompatible destination: another asset (BEZ_FLAG_CLEATS / BEZ_FLAG_BOX_ASSET)");
    if (d->has_ball != o->has_ball) return fail(d, -1, "bez_snapshot_restore: incompatible destination: ball / no ball");
    if (d->nobs != o->nobs) return fail(d, -1, "bez_snapshot_restore: incompatible destination: another observation width");
  }
  const bool globals = (what & BEZ_SNAPSHOT_GLOBALS) != 0u;
  if (count == 0 && !globals) return 0;
  (void)hipSetDevice(d->device);
  int mode[BEZ_SNAPSHOT_SECTIONS];
  bool packed = false, gravity = false;
  for (int k = 0; k < BEZ_SNAPSHOT_SECTIONS; ++k) {
    const bool in_snap = (p->present >> k) & 1u;
    const int param = k >= SNAP_SEC_PARAM0 && k < SNAP_SEC_DF ? k - SNAP_SEC_PARAM0 : -1;
    if (param >= 0 && in_snap && !d->dr[param] && count > 0) {   // the path of bez_sim_set_env_params: default rows for the envs not restored
      RC_TRY(dev_alloc_zeroed(d, &d->dr[param], (size_t)d->n * PARAM_WIDTH[param] * sizeof(float), stream));
      if (int rc = fill_default_params(d, param, d->dr[param], stream)) { dev_free(d, &d->dr[param]); return rc; }
    }
    const bool in_dst = SNAP_TABLE[k].env(d) != nullptr && snap_width(d, k) == p->width[k];
    mode[k] = count == 0 ? SNAP_SKIP : (in_snap && in_dst) ? SNAP_COPY : (param >= 0 && in_dst) ? SNAP_DEFAULT : SNAP_SKIP;
    if (param >= 0 && mode[k] != SNAP_SKIP) {
      packed |= param == BEZ_PARAM_KP_SCALE || param == BEZ_PARAM_KD_SCALE || param == BEZ_PARAM_DOF_LOWER || param == BEZ_PARAM_DOF_UPPER;
      gravity |= param == BEZ_PARAM_GRAVITY;
    }
  }
  RC_TRY(launch_snapshot<false>(d, p, mode, env_ids_dev, row_ids_dev, count, globals, stream));
  if (packed && repack_dr(d, stream)) return fail(d, -2, "bez_snapshot_restore: repack");
  if (gravity) d->gravity_uniform = false;   // rows written from outside the randomisation kernel may differ from env to env
  if (globals) {
    d->obs_calls = p->obs_calls; d->post_calls = p->post_calls; d->reset_calls = p->reset_calls;
    d->gravity_uniform = p->gravity_uniform != 0u; d->obs_noise_applied = p->obs_noise_applied != 0u;
  }
  return 0;
}
int bez_snapshot_export(BezSim* s, const BezSnapshot* p, void* blob, int64_t* bytes, void* stream_) {
  SNAP_TRY(s, p, "bez_snapshot_export", true);
  if (!bytes) return fail(s, -1, "bez_snapshot_export: bytes is null");
  const int64_t need = (int64_t)((BEZ_SNAPSHOT_HEADER_WORDS + snap_words(p)) * sizeof(uint32_t)), room = *bytes;
  *bytes = need;
  if (!blob) return 0;
  if (room < need) return fail(s, -1, "bez_snapshot_export: the blob is too small (*bytes is the size needed)");
  hipStream_t stream = (hipStream_t)stream_;
  uint32_t h[BEZ_SNAPSHOT_HEADER_WORDS];
  snap_header(s, p, h);
  (void)hipSetDevice(s->device);
  HIP_TRY(s, hipMemcpyAsync(blob, h, sizeof(h), hipMemcpyDefault, stream));
  HIP_TRY(s, hipMemcpyAsync((uint32_t*)blob + BEZ_SNAPSHOT_HEADER_WORDS, p->data, snap_words(p) * sizeof(uint32_t), hipMemcpyDefault, stream));
  HIP_TRY(s, hipStreamSynchronize(stream));
  return 0;
}
int bez_snapshot_import(BezSim* s, BezSnapshot* p, const void* blob, int64_t bytes, void* stream_) {
  SNAP_TRY(s, p, "bez_snapshot_import", true);
  if (!blob) return fail(s, -1, "bez_snapshot_import: blob is null");
  const int64_t need = (int64_t)((BEZ_SNAPSHOT_HEADER_WORDS + snap_words(p)) * sizeof(uint32_t));
  if (bytes < (int64_t)(BEZ_SNAPSHOT_HEADER_WORDS * sizeof(uint32_t))) return fail(s, -1, "bez_snapshot_import: the blob is truncated (shorter than its header)");
  hipStream_t stream = (hipStream_t)stream_;
  (void)hipSetDevice(s->device);
  uint32_t h[BEZ_SNAPSHOT_HEADER_WORDS], mine[BEZ_SNAPSHOT_HEADER_WORDS];
  HIP_TRY(s, hipMemcpyAsync(h, blob, sizeof(h), hipMemcpyDefault, stream));
  HIP_TRY(s, hipStreamSynchronize(stream));
  snap_header(s, p, mine);
  if (h[0] != BEZ_SNAPSHOT_MAGIC) return fail(s, -1, "bez_snapshot_import: not a snapshot blob (magic word)");
  if (h[1] != BEZ_SNAPSHOT_LAYOUT) return fail(s, -1, "bez_snapshot_import: the blob has another layout version");
  if (h[2] != mine[2]) return fail(s, -1, "bez_snapshot_import: the blob has another number of rows");
  if (h[3] != mine[3] || h[5] != mine[5] || h[6] != mine[6] || std::memcmp(h + 8, mine + 8, BEZ_SNAPSHOT_SECTIONS * sizeof(uint32_t)) != 0)
    return fail(s, -1, "bez_snapshot_import: the blob's section widths do not fit this snapshot");
  const uint32_t *g = h + 8 + BEZ_SNAPSHOT_SECTIONS, *gm = mine + 8 + BEZ_SNAPSHOT_SECTIONS;
  if (std::memcmp(g + 8, gm + 8, 4 * sizeof(uint32_t)) != 0) return fail(s, -1, "bez_snapshot_import: the blob is of another task or asset");
  if (bytes < need) return fail(s, -1, "bez_snapshot_import: the blob is truncated");
  HIP_TRY(s, hipMemcpyAsync(p->data, (const uint32_t*)blob + BEZ_SNAPSHOT_HEADER_WORDS, snap_words(p) * sizeof(uint32_t), hipMemcpyDefault, stream));
  HIP_TRY(s, hipStreamSynchronize(stream));
  p->present = h[4];
  p->obs_calls = (int64_t)((uint64_t)g[0] | (uint64_t)g[1] << 32); p->post_calls = (uint64_t)g[2] | (uint64_t)g[3] << 32;
  p->reset_calls = (uint64_t)g[4] | (uint64_t)g[5] << 32; p->gravity_uniform = g[6]; p->obs_noise_applied = g[7];
  return 0;
}
}  // extern "C"
