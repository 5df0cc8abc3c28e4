// bez_dynamics.h -- the kernels that run forward kinematics outside the control step (rigid-body refresh, dynamics tensors, inverse, forward and
// centroidal dynamics, body accelerations, external wrenches, limb inverse kinematics, operational space, proximity), and the kernel that fills
// a query state, the second state they can be run on.  Included by bez_sim.hip only.
// What they share, each defined once and named, not restated, in the kernels' own comments:
//   body_frame, for_each_body_of_link      a body's link, offset and centre of mass; the bodies fixed to one link
//   chain_first / chain_len, for_each_chain the tree's five chains off the torso, derived from BEZ_LINK_PARENT, in either order
//   still_chain_walk                        a chain's link frames and joint axes with the joints standing still
//   DynArgs, mass_scale_of, gravity_of      what the host tells every kernel about the sim; the parameter rows
//   state_at, state3_at, root_rotation      single fields of an env's state (load_state / link_frames: all of it)
//   tile_load, tile_store, tile_load_or_zero  a tile's rows between LDS and one contiguous global range, any row width
//   link_inertias, composite_sweep          the composite-rigid-body front end of the mass and momentum matrices
//   mass_slots (MASS_SLOT_TABLE, MASS_SLOTS) where every entry of M lives among an env's distinct words
//   chol_factor, chol_solve                 a register-resident Cholesky solve of up to 6 x 6
#pragma once
#include "bez_kernels.h"

namespace bez {

BEZ_DEV void mat_to_quat(const M3& R, float q[4]) {
  float tr = R.m00 + R.m11 + R.m22;
  if (tr > 0.f) {
    float s = sqrtf(tr + 1.f) * 2.f;
    q[3] = 0.25f * s; q[0] = (R.m21 - R.m12) / s; q[1] = (R.m02 - R.m20) / s; q[2] = (R.m10 - R.m01) / s;
  } else if (R.m00 > R.m11 && R.m00 > R.m22) {
    float s = sqrtf(1.f + R.m00 - R.m11 - R.m22) * 2.f;
    q[3] = (R.m21 - R.m12) / s; q[0] = 0.25f * s; q[1] = (R.m01 + R.m10) / s; q[2] = (R.m02 + R.m20) / s;
  } else if (R.m11 > R.m22) {
    float s = sqrtf(1.f + R.m11 - R.m00 - R.m22) * 2.f;
    q[3] = (R.m02 - R.m20) / s; q[0] = (R.m01 + R.m10) / s; q[1] = 0.25f * s; q[2] = (R.m12 + R.m21) / s;
  } else {
    float s = sqrtf(1.f + R.m22 - R.m00 - R.m11) * 2.f;
    q[3] = (R.m10 - R.m01) / s; q[0] = (R.m02 + R.m20) / s; q[1] = (R.m12 + R.m21) / s; q[2] = 0.25f * s;
  }
}

// Forward kinematics of one env's link frames: orientation E[l] and origin r[l] (relative to the root's position) of every link, and
// WITH_VEL the spatial velocities V[l] (without: V is scratch, the joints stand still)
template <bool CL, bool WITH_VEL>
BEZ_DEV void link_frames(const EnvState& S, uint32_t flags, M3 (&E)[BEZ_NL], V3 (&r)[BEZ_NL], SV (&V)[BEZ_NL]) {
  E[0] = quat_to_mat(S.rq[0], S.rq[1], S.rq[2], S.rq[3]);
  r[0] = mk(0, 0, 0);
  V[0] = WITH_VEL ? mksv(S.root_ang, S.root_lin) : svzero();
  static_for<BEZ_NL - 1>([&](auto I) {
    constexpr int L = 1 + decltype(I)::value;
    constexpr int p = BEZ_LINK_PARENT[L];
    E[L] = E[p]; r[L] = r[p]; V[L] = V[p];
    SV Sj, cb;
    link_kinematics<L>(S.q[L - 1], WITH_VEL ? S.qd[L - 1] : 0.f, E[L], r[L], V[L], Sj, cb, quirk_rz<CL>(flags));
  });
}
// Robot body b of the asset: the link it is fixed to, its origin's offset in that link's frame, its centre of mass in its own frame
struct BodyFrame { int link; V3 off, com; };
template <bool CL>
BEZ_DEV BodyFrame body_frame(int b) {
  // (the offsets are handed out as floats, and "the body sits at its link's origin" is asked of those: none may vanish only in float)
  static_assert([] {
    for (int i = 0; i < nb_of<CL>(); ++i)
      for (int k = 0; k < 3; ++k) {
        const double v = CL ? BEZ_BODY_OFFSET_CL[i][k] : BEZ_BODY_OFFSET[i][k];
        if (v != 0.0 && (float)v == 0.f) return false;
      }
    return true;
  }(), "a body offset component is non-zero in double and zero in float");
  const double* o = CL ? BEZ_BODY_OFFSET_CL[b] : BEZ_BODY_OFFSET[b];
  const double* c = CL ? BEZ_BODY_COM_CL[b] : BEZ_BODY_COM[b];
  return {CL ? BEZ_BODY_LINK_CL[b] : BEZ_BODY_LINK[b], mk((float)o[0], (float)o[1], (float)o[2]), mk((float)c[0], (float)c[1], (float)c[2])};
}
// The bodies fixed to link L, in the order of their indices: each(b as an integral constant, its BodyFrame, whether its origin is the link's)
template <bool CL, int L, typename Each>
BEZ_DEV void for_each_body_of_link(Each&& each) {
  static_for<nb_of<CL>()>([&](auto I) {
    constexpr int b = decltype(I)::value;
    if constexpr ((CL ? BEZ_BODY_LINK_CL[b] : BEZ_BODY_LINK[b]) == L) {
      const BodyFrame bf = body_frame<CL>(b);
      each(I, bf, bf.off.x == 0.f && bf.off.y == 0.f && bf.off.z == 0.f);
    }
  });
}

// The tree is a torso (link 0) and BEZ_IK_CHAINS chains off it.  Chain c: the c-th link whose parent is the torso, and the links after
// it up to the next such link.  for_each_chain hands every chain's (FIRST, LEN) to f as integral constants, first to last or
// LAST_FIRST; the kernels that walk the tree lane by lane take the chains one after the other through it.
template <int FIRST, int LEN> constexpr bool is_chain() {
  if (BEZ_LINK_PARENT[FIRST] != 0) return false;
  for (int i = 1; i < LEN; ++i) if (BEZ_LINK_PARENT[FIRST + i] != FIRST + i - 1) return false;
  return FIRST + LEN == BEZ_NL || BEZ_LINK_PARENT[FIRST + LEN] == 0;
}
constexpr int chain_first(int c) { for (int l = 1; l < BEZ_NL; ++l) if (BEZ_LINK_PARENT[l] == 0 && c-- == 0) return l; return -1; }
constexpr int chain_len(int c) { const int f = chain_first(c); int k = 1; while (f + k < BEZ_NL && BEZ_LINK_PARENT[f + k] != 0) ++k; return k; }
static_assert(chain_first(BEZ_IK_CHAINS - 1) > 0 && chain_first(BEZ_IK_CHAINS) < 0, "BEZ_IK_CHAINS chains off the torso");
static_assert(chain_first(0) == 1 && chain_len(0) == 2 && chain_first(1) == 3 && chain_len(1) == 2 && chain_first(2) == 5 && chain_len(2) == 6 &&
              chain_first(3) == 11 && chain_len(3) == 2 && chain_first(4) == 13 && chain_len(4) == 6, "head, two arms, two legs: (1,2) (3,2) (5,6) (11,2) (13,6)");
template <bool LAST_FIRST, typename F>
BEZ_DEV void for_each_chain(F&& f) {
  static_for<BEZ_IK_CHAINS>([&](auto I) {
    constexpr int c = LAST_FIRST ? BEZ_IK_CHAINS - 1 - decltype(I)::value : decltype(I)::value;
    // (this one assertion covers the kernels that take chain c by its index, too: some kernel of this header always comes through here)
    static_assert(is_chain<chain_first(c), chain_len(c)>(), "not a chain off the torso");
    f(std::integral_constant<int, chain_first(c)>{}, std::integral_constant<int, chain_len(c)>{});
  });
}
// A chain walked with its joints standing still (link_kinematics at qd = 0), from the frame (E, r), which is left as the last link's:
// q(L) is link L's joint angle, each(L, S) sees the link's frame in E, r and its joint's motion axis S = [a; r x a]
template <int FIRST, int LEN, typename Angle, typename Each>
BEZ_DEV void still_chain_walk(M3& E, V3& r, float quirk_z, Angle&& q, Each&& each) {
  static_for<LEN>([&](auto I) {
    constexpr int L = FIRST + decltype(I)::value;
    SV S, cb, V = svzero();
    link_kinematics<L>(q(std::integral_constant<int, L>{}), 0.f, E, r, V, S, cb, quirk_z);
    each(std::integral_constant<int, L>{}, S);
  });
}

// gym.refresh_rigid_body_state_tensor: forward kinematics of all 21 robot bodies + the ball row
template <bool CL>
__global__ void refresh_rigid_body_kernel(const float* __restrict__ st, float* __restrict__ out, int n, int has_ball, uint32_t flags) {
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  EnvState S;
  load_state(st, n, e, S);
  M3 E[BEZ_NL]; V3 r[BEZ_NL]; SV V[BEZ_NL];
  link_frames<CL, true>(S, flags, E, r, V);
  constexpr int NB = nb_of<CL>();
  const int nbe = NB + (has_ball ? 1 : 0);
  static_for<NB>([&](auto I) {
    const BodyFrame f = body_frame<CL>(decltype(I)::value);
    const int b = decltype(I)::value, l = f.link;
    V3 x = r[l] + mul(E[l], f.off);
    V3 vel = point_of(V[l], x);
    float q[4];
    mat_to_quat(E[l], q);
    float* o = out + ((size_t)e * nbe + b) * 13;
    o[0] = S.root_pos.x + x.x; o[1] = S.root_pos.y + x.y; o[2] = S.root_pos.z + x.z;
    o[3] = q[0]; o[4] = q[1]; o[5] = q[2]; o[6] = q[3];
    o[7] = vel.x; o[8] = vel.y; o[9] = vel.z; o[10] = V[l].a.x; o[11] = V[l].a.y; o[12] = V[l].a.z;
  });
  if (!has_ball) return;
  float* o = out + ((size_t)e * nbe + NB) * 13;
  o[0] = S.ball_pos.x; o[1] = S.ball_pos.y; o[2] = S.ball_pos.z;
  o[3] = S.bq[0]; o[4] = S.bq[1]; o[5] = S.bq[2]; o[6] = S.bq[3];
  o[7] = S.ball_lin.x; o[8] = S.ball_lin.y; o[9] = S.ball_lin.z; o[10] = S.ball_ang.x; o[11] = S.ball_ang.y; o[12] = S.ball_ang.z;
}

// ---- gym.refresh_jacobian_tensors / gym.refresh_mass_matrix_tensors (definitions: include/bez_sim.h "Dynamics tensors").
// A workgroup takes DYN_TILE consecutive envs.  Phase 1, one lane per env: forward kinematics, then the world joint axes, the joint
// origins and the body origins (both relative to the root origin) go to LDS, and -- still in that lane -- the composite-rigid-body
// recursion in the frame link_inertia already uses (world axes about the root origin: composites add up without transforms) leaves
// every DISTINCT entry of M in LDS.  Phase 2, all lanes: the tile's output range is contiguous (DYN_TILE x nb x 144 floats of J,
// DYN_TILE x 576 of M), and each lane forms four consecutive elements from LDS and stores them as one float4, so every store
// instruction of a wave covers 1 KB of consecutive addresses.  Structural zeros and ones are constants, never computed.
constexpr int DYN_TILE = 16, DYN_THREADS = 256, DYN_NG = 6 + BEZ_ND;
constexpr int link_depth(int l) { int d = 0; for (; l > 0; l = BEZ_LINK_PARENT[l]) ++d; return d; }
constexpr int dyn_pair_base(int l) { int s = 0; for (int k = 1; k < l; ++k) s += link_depth(k); return s; }   // (l, its path to the root) starts here
constexpr uint32_t link_ancestors(int l) { uint32_t m = 0; for (; l > 0; l = BEZ_LINK_PARENT[l]) m |= 1u << l; return m; }   // bit l' : DOF l' - 1 moves link l
// LDS words of one env: [axis 18x3][joint origin 18x3][body origin nb x 3][the distinct entries of M]
constexpr int DYN_AX = 0, DYN_RO = 3 * BEZ_ND, DYN_XB = 6 * BEZ_ND, DYN_MS = DYN_XB + 3 * BEZ_NB_CL;
// entries of M: 0 the constant zero, total mass, h, -h, Ibar (xx yy zz xy xz yz), F_l = I^c_l S_l as [lin; ang] per joint, S_j . F_l per path pair
constexpr int MS_ZERO = 0, MS_MASS = 1, MS_H = 2, MS_NH = 5, MS_IBAR = 8, MS_F = 14, MS_PAIR = MS_F + 6 * BEZ_ND, MS_COUNT = MS_PAIR + dyn_pair_base(BEZ_NL);
constexpr int DYN_STRIDE = (DYN_MS + MS_COUNT) | 1;   // odd: the lanes of phase 1 (one env each) write distinct banks
struct MassSlots { int16_t s[DYN_NG * DYN_NG]; };
constexpr MassSlots mass_slots() {
  MassSlots T = {};
  for (int i = 0; i < DYN_NG * DYN_NG; ++i) T.s[i] = MS_ZERO;
  const int ibar[3][3] = {{0, 3, 4}, {3, 1, 5}, {4, 5, 2}};
  // skew(h) = [[0, -hz, hy], [hz, 0, -hx], [-hy, hx, 0]] as (component, negated)
  const int sk[3][3] = {{-1, MS_NH + 2, MS_H + 1}, {MS_H + 2, -1, MS_NH + 0}, {MS_NH + 1, MS_H + 0, -1}};
  for (int r = 0; r < 3; ++r) {
    T.s[r * DYN_NG + r] = MS_MASS;
    for (int c = 0; c < 3; ++c) {
      T.s[(3 + r) * DYN_NG + 3 + c] = (int16_t)(MS_IBAR + ibar[r][c]);
      if (sk[r][c] >= 0) T.s[(3 + r) * DYN_NG + c] = T.s[c * DYN_NG + 3 + r] = (int16_t)sk[r][c];   // ang row, lin column = skew(h); its transpose
    }
  }
  for (int l = 1; l < BEZ_NL; ++l) {
    for (int k = 0; k < 6; ++k) T.s[(5 + l) * DYN_NG + k] = T.s[k * DYN_NG + 5 + l] = (int16_t)(MS_F + 6 * (l - 1) + k);
    int p = MS_PAIR + dyn_pair_base(l);
    for (int j = l; j > 0; j = BEZ_LINK_PARENT[j], ++p) T.s[(5 + l) * DYN_NG + 5 + j] = T.s[(5 + j) * DYN_NG + 5 + l] = (int16_t)p;
  }
  return T;
}
constexpr MassSlots MASS_SLOT_TABLE = mass_slots();        // for compile-time indices (mass_at)
__device__ const MassSlots MASS_SLOTS = MASS_SLOT_TABLE;   // for run-time ones (phase 2 of refresh_dynamics_kernel)
struct BodyAncestors { uint32_t m[BEZ_NB_CL]; };
template <bool CL> constexpr BodyAncestors body_ancestors() {
  BodyAncestors T = {};
  for (int b = 0; b < (CL ? BEZ_NB_CL : BEZ_NB); ++b) T.m[b] = link_ancestors(CL ? BEZ_BODY_LINK_CL[b] : BEZ_BODY_LINK[b]);
  return T;
}
template <bool CL> __device__ const BodyAncestors BODY_ANCESTORS = body_ancestors<CL>();

BEZ_DEV float pick(V3 v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : v.z); }
BEZ_DEV V3 lds3(const float* p) { return mk(p[0], p[1], p[2]); }
// J[row][col] of a body with origin x (relative to the root origin) whose link has the ancestor set `mask`; L: the env's LDS words
BEZ_DEV float jacobian_entry(const float* L, uint32_t mask, V3 x, int row, int col) {
  if (col < 3) return row == col ? 1.f : 0.f;
  if (col < 6) {
    if (row >= 3) return row == col ? 1.f : 0.f;
    const int c = col - 3;                      // -skew(x) = [[0, z, -y], [-z, 0, x], [y, -x, 0]]
    if (c == row) return 0.f;
    const float v = pick(x, 3 - row - c);
    return ((c - row + 3) % 3 == 1) ? v : -v;
  }
  const int d = col - 6;
  if (!((mask >> (d + 1)) & 1u)) return 0.f;
  const V3 a = lds3(L + DYN_AX + 3 * d);
  if (row >= 3) return pick(a, row - 3);
  return pick(cross(a, x - lds3(L + DYN_RO + 3 * d)), row);
}

// What the three dynamics kernels are told about the sim (the host's dyn_args): the SoA state, the BEZ_PARAM_MASS_SCALE and BEZ_PARAM_GRAVITY
// rows they share with the step (null: the defaults) and the config's scalars
struct DynArgs { const float *st, *mass_scale, *gravity_rows; int n; uint32_t flags; float armature, g[3]; };
// link l's BEZ_PARAM_MASS_SCALE entry (1 without rows) and the env's BEZ_PARAM_GRAVITY row (the config's vector without rows)
BEZ_DEV float mass_scale_of(const DynArgs& D, int e, int l) { return D.mass_scale ? D.mass_scale[(size_t)e * BEZ_NL + l] : 1.f; }
BEZ_DEV V3 gravity_of(const DynArgs& D, int e) {
  return D.gravity_rows ? mk(D.gravity_rows[(size_t)e * 3], D.gravity_rows[(size_t)e * 3 + 1], D.gravity_rows[(size_t)e * 3 + 2]) : mk(D.g[0], D.g[1], D.g[2]);
}

// The state of env e: field f of the SoA state, three consecutive fields as a vector, the root's orientation.  For the kernels that read
// a few fields where they need them; load_state / link_frames bring in all of it.
BEZ_DEV float state_at(const DynArgs& D, int f, int e) { return D.st[(size_t)f * D.n + e]; }
BEZ_DEV V3 state3_at(const DynArgs& D, int f, int e) { return mk(state_at(D, f, e), state_at(D, f + 1, e), state_at(D, f + 2, e)); }
BEZ_DEV M3 root_rotation(const DynArgs& D, int e) {
  return quat_to_mat(state_at(D, F_ROOT_QUAT, e), state_at(D, F_ROOT_QUAT + 1, e), state_at(D, F_ROOT_QUAT + 2, e), state_at(D, F_ROOT_QUAT + 3, e));
}

// Tile I/O: `nrows` rows of WIDTH floats between LDS (`rows`, STRIDE words apart) and the contiguous global range at `in` / `out`, by a
// workgroup of THREADS lanes.  A range that starts 16-byte aligned moves as float4, with a scalar tail of (nrows * WIDTH) % 4 elements
// where rows are not whole float4s; any other takes the scalar path to the same bits.  tile_load_or_zero: zeros where there is no input.
template <int WIDTH, int STRIDE>
BEZ_DEV int tile_word(int i) { return (i / WIDTH) * STRIDE + i % WIDTH; }   // where element i of the global range lives in LDS
template <int WIDTH, int STRIDE, int THREADS>
BEZ_DEV void tile_load(float* rows, const float* __restrict__ in, int nrows) {
  auto slot = [&](int i) -> float& { return rows[tile_word<WIDTH, STRIDE>(i)]; };
  const int count = nrows * WIDTH;
  if ((reinterpret_cast<uintptr_t>(in) & 15u) == 0) {
    const float4* in4 = reinterpret_cast<const float4*>(in);
    const int n4 = count / 4;
    for (int i = threadIdx.x; i < n4; i += THREADS) {
      const float4 v = in4[i];
      slot(4 * i) = v.x; slot(4 * i + 1) = v.y; slot(4 * i + 2) = v.z; slot(4 * i + 3) = v.w;
    }
    if constexpr (WIDTH % 4 != 0) {
      for (int i = 4 * n4 + threadIdx.x; i < count; i += THREADS) slot(i) = in[i];
    }
  } else {
    for (int i = threadIdx.x; i < count; i += THREADS) slot(i) = in[i];
  }
}
template <int WIDTH, int STRIDE, int THREADS>
BEZ_DEV void tile_store(const float* rows, float* __restrict__ out, int nrows) {
  auto at = [&](int i) { return rows[tile_word<WIDTH, STRIDE>(i)]; };
  const int count = nrows * WIDTH;
  if ((reinterpret_cast<uintptr_t>(out) & 15u) == 0) {
    float4* o4 = reinterpret_cast<float4*>(out);
    const int n4 = count / 4;
    for (int i = threadIdx.x; i < n4; i += THREADS) o4[i] = make_float4(at(4 * i), at(4 * i + 1), at(4 * i + 2), at(4 * i + 3));
    if constexpr (WIDTH % 4 != 0) {
      for (int i = 4 * n4 + threadIdx.x; i < count; i += THREADS) out[i] = at(i);
    }
  } else {
    for (int i = threadIdx.x; i < count; i += THREADS) out[i] = at(i);
  }
}
template <int WIDTH, int STRIDE, int THREADS>
BEZ_DEV void tile_load_or_zero(float* rows, const float* in, int nrows) {
  if (in) {
    tile_load<WIDTH, STRIDE, THREADS>(rows, in, nrows);
  } else {
    for (int i = threadIdx.x; i < nrows * WIDTH; i += THREADS) rows[tile_word<WIDTH, STRIDE>(i)] = 0.f;
  }
}

// ---- query states (definitions: include/bez_sim.h "Query states"): a second SoA state of `rows` rows for the kernels of this header,
// with row-by-row copies of the four parameter rows they read.  The SoA stops where the fields no query reads begin (targets, previous
// velocity, contact forces, feet, goal): load_state and every state_at of this header stay below F_TARGET.  A query that starts to read
// a field behind the cut has to move QS_FIELDS -- the assertion ties the cut to the layout, so that a field inserted in front of it or
// a reordering cannot leave such a read outside the allocation unnoticed.
constexpr int QS_FIELDS = F_TARGET;
static_assert(F_ROOT_POS == 0 && F_Q == 13 && F_QD == F_Q + BEZ_ND && F_BALL_POS == F_QD + BEZ_ND && F_BALL_ANG + 3 == QS_FIELDS &&
              F_PREV > F_TARGET && F_CF > F_TARGET && F_FEET > F_TARGET && F_GOAL > F_TARGET && QS_FIELDS < F_COUNT,
              "a query state holds root 13, q 18, qd 18, ball 13 in the sim's field order, and nothing a query reads lies behind them");
constexpr int QS_PARAMS = 4;
constexpr int QS_PARAM_ID[QS_PARAMS] = {BEZ_PARAM_MASS_SCALE, BEZ_PARAM_GRAVITY, BEZ_PARAM_DOF_LOWER, BEZ_PARAM_DOF_UPPER};
constexpr int QS_PARAM_WIDTH[QS_PARAMS] = {BEZ_NL, 3, BEZ_ND, BEZ_ND};
// What the host tells the fill kernels.  dst: the query state; src: the sim's parameter rows (null: never allocated) and, for a capture,
// its SoA state of n envs; root / dof / ball: the Isaac-layout rows of a set (ball null: ball_rest, the config's pose, at rest);
// ids: the env of every row (null: none for a set, the row's own index for a capture); g: the config's gravity
struct QsFill {
  float* st; int rows;
  float* param[QS_PARAMS];
  const float* src_param[QS_PARAMS];
  const float* src_st; int n;
  const float *root, *dof, *ball;
  const int32_t* ids;
  float ball_rest[7], g[3];
};
// bez_query_state_set (CAPTURE false) and bez_query_state_capture (true).  A workgroup takes QS_TILE consecutive rows.
// Set: all lanes bring the tile's root, DOF and ball rows -- three contiguous ranges -- into LDS with tile_load, side by side in one staged
// row per env in the sim's field order (the DOF words stay interleaved [q0, qd0, q1, ...] as DOF_STATE has them: qs_word finds a field);
// then consecutive lanes write consecutive rows of ONE field, so a wave's store is one contiguous 256-byte range of that SoA column, and
// its LDS reads are QS_STRIDE (odd) words apart: distinct banks.  Capture: SoA to SoA, the same column writes; the reads are the gather
// by env id itself (contiguous for the identity).  Both: the parameter rows, written as one contiguous range per parameter and read row
// by row from env ids[i] -- an id outside 0 .. n-1 (or a parameter the sim never allocated) takes the default row in a set, and leaves
// the whole row, state and parameters, as it is in a capture.  Values are copied as they are.
constexpr int QS_TILE = 64, QS_THREADS = 256, QS_STRIDE = QS_FIELDS | 1;
BEZ_DEV int qs_word(int f) { return f < F_Q ? f : f < F_QD ? F_Q + 2 * (f - F_Q) : f < F_BALL_POS ? F_Q + 2 * (f - F_QD) + 1 : f; }
template <bool CAPTURE>
__global__ void __launch_bounds__(QS_THREADS) query_state_fill_kernel(QsFill A) {
  __shared__ float staged[CAPTURE ? 1 : QS_TILE * QS_STRIDE];
  __shared__ int env[QS_TILE];
  const int r0 = blockIdx.x * QS_TILE, nr = min(QS_TILE, A.rows - r0);
  for (int r = threadIdx.x; r < nr; r += QS_THREADS) {
    const int e = A.ids ? A.ids[r0 + r] : (CAPTURE ? r0 + r : -1);
    env[r] = (e >= 0 && e < A.n) ? e : -1;
  }
  if constexpr (!CAPTURE) {
    tile_load<13, QS_STRIDE, QS_THREADS>(staged + F_ROOT_POS, A.root + (size_t)r0 * 13, nr);
    tile_load<2 * BEZ_ND, QS_STRIDE, QS_THREADS>(staged + F_Q, A.dof + (size_t)r0 * 2 * BEZ_ND, nr);
    if (A.ball) {
      tile_load<13, QS_STRIDE, QS_THREADS>(staged + F_BALL_POS, A.ball + (size_t)r0 * 13, nr);
    } else {
      for (int i = threadIdx.x; i < nr * 13; i += QS_THREADS) staged[F_BALL_POS + tile_word<13, QS_STRIDE>(i)] = i % 13 < 7 ? A.ball_rest[i % 13] : 0.f;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < QS_FIELDS * QS_TILE; i += QS_THREADS) {
    const int f = i / QS_TILE, r = i % QS_TILE;
    if (r >= nr) continue;
    float* dst = A.st + (size_t)f * A.rows + r0 + r;
    if constexpr (CAPTURE) {
      if (env[r] >= 0) *dst = A.src_st[(size_t)f * A.n + env[r]];
    } else {
      *dst = staged[r * QS_STRIDE + qs_word(f)];
    }
  }
  static_for<QS_PARAMS>([&](auto P) {
    constexpr int p = decltype(P)::value, W = QS_PARAM_WIDTH[p];
    const float* src = A.src_param[p];
    float* dst = A.param[p] + (size_t)r0 * W;
    for (int i = threadIdx.x; i < nr * W; i += QS_THREADS) {
      const int e = env[i / W], k = i % W;
      if (CAPTURE && e < 0) continue;
      const float nominal = p == 0 ? 1.f : p == 1 ? (k == 0 ? A.g[0] : k == 1 ? A.g[1] : A.g[2]) : p == 2 ? (float)BEZ_DOF_LOWER[k] : (float)BEZ_DOF_UPPER[k];
      dst[i] = (src && e >= 0) ? src[(size_t)e * W + k] : nominal;
    }
  });
}

// The composite-rigid-body front end of the mass matrix and of the momentum matrix, in the frame link_inertia uses (world axes about the
// root origin: composites add up without transforms).  link_inertias: every link's own inertia for env e, joints at rest, no gravity;
// each(l) follows link l's inertia (the centroidal kernel's kinetic energy: summed in a loop of its own it cost 14 VGPRs and 0.1 us).
// composite_sweep, leaves first: link l is complete when its turn comes; each(l, F_l) sees F_l = I^c_l S_l, S_l = [a; r x a] with
// a the joint's axis, then the link joins its parent.  Ic[0] ends as the whole robot's inertia.
BEZ_DEV SV inertia_times(const LinkInertia& I, SV a) {   // I a = [Ibar a.a + h x a.l ; m a.l - h x a.a]
  return mksv(mul(I.Ibar, a.a) + cross(I.h, a.l), a.l * I.m - cross(I.h, a.a));
}
template <bool CL, typename Each>
BEZ_DEV void link_inertias(const DynArgs& D, int e, const M3 (&E)[BEZ_NL], const V3 (&r)[BEZ_NL], LinkInertia (&Ic)[BEZ_NL], Each&& each) {
  static_for<BEZ_NL>([&](auto I) {
    constexpr int l = decltype(I)::value;
    SV pA;
    link_inertia<l, CL>(mass_scale_of(D, e, l), mk(0, 0, 0), E[l], r[l], svzero(), Ic[l], pA);
    each(I);
  });
}
template <typename Each>
BEZ_DEV void composite_sweep(LinkInertia (&Ic)[BEZ_NL], const M3 (&E)[BEZ_NL], const V3 (&r)[BEZ_NL], Each&& each) {
  static_for<BEZ_NL - 1>([&](auto I) {
    constexpr int l = BEZ_NL - 1 - decltype(I)::value, p = BEZ_LINK_PARENT[l];
    const LinkInertia& C = Ic[l];
    const V3 a = col(E[l], axis_index(l)) * axis_sign(l);   // the column of the link's frame that the joint rotation leaves alone
    each(std::integral_constant<int, l>{}, inertia_times(C, mksv(a, cross(r[l], a))));
    Ic[p].m += C.m; Ic[p].h = Ic[p].h + C.h; add_to(Ic[p].Ibar, C.Ibar);
  });
}

// Phase 1 for one env, shared with forward_dynamics_kernel.  L: the env's LDS words; E, r: its link frames (link_frames).
// dyn_joint_words: the world joint axes and the joint origins; dyn_mass_words, which reads them back: the distinct entries of M
// (without PAIRS: the base block and the F_l alone).
BEZ_DEV void dyn_put3(float* L, int at, V3 v) { L[at] = v.x; L[at + 1] = v.y; L[at + 2] = v.z; }
BEZ_DEV void dyn_joint_words(float* L, const M3 (&E)[BEZ_NL], const V3 (&r)[BEZ_NL]) {
  static_for<BEZ_ND>([&](auto I) {   // the joint's axis is the column of its link's frame that the joint rotation leaves alone
    constexpr int l = 1 + decltype(I)::value;
    dyn_put3(L, DYN_AX + 3 * (l - 1), col(E[l], axis_index(l)) * axis_sign(l));
    dyn_put3(L, DYN_RO + 3 * (l - 1), r[l]);
  });
}
template <bool CL, bool PAIRS = true>
BEZ_DEV void dyn_mass_words(const DynArgs& D, int e, float* L, const M3 (&E)[BEZ_NL], const V3 (&r)[BEZ_NL]) {
  LinkInertia Ic[BEZ_NL];
  link_inertias<CL>(D, e, E, r, Ic, [](auto) {});
  float* Ms = L + DYN_MS;
  composite_sweep(Ic, E, r, [&](auto Lk, SV F) {
    constexpr int l = decltype(Lk)::value;
    dyn_put3(L, DYN_MS + MS_F + 6 * (l - 1), F.l);
    dyn_put3(L, DYN_MS + MS_F + 6 * (l - 1) + 3, F.a);
    if constexpr (PAIRS) {
      int at = MS_PAIR + dyn_pair_base(l);
      for (int j = l; j > 0; j = BEZ_LINK_PARENT[j], ++at) {
        const V3 aj = lds3(L + DYN_AX + 3 * (j - 1)), sj = cross(lds3(L + DYN_RO + 3 * (j - 1)), aj);
        const float v = dot(aj, F.a) + dot(sj, F.l);
        Ms[at] = j == l ? v + D.armature : v;
      }
    }
  });
  const LinkInertia& C = Ic[0];
  Ms[MS_ZERO] = 0.f; Ms[MS_MASS] = C.m;
  dyn_put3(L, DYN_MS + MS_H, C.h); dyn_put3(L, DYN_MS + MS_NH, -C.h);
  Ms[MS_IBAR] = C.Ibar.xx; Ms[MS_IBAR + 1] = C.Ibar.yy; Ms[MS_IBAR + 2] = C.Ibar.zz;
  Ms[MS_IBAR + 3] = C.Ibar.xy; Ms[MS_IBAR + 4] = C.Ibar.xz; Ms[MS_IBAR + 5] = C.Ibar.yz;
}

template <bool CL>
__global__ void __launch_bounds__(DYN_THREADS) refresh_dynamics_kernel(DynArgs D, float* __restrict__ J, float* __restrict__ M) {
  __shared__ float lds[DYN_TILE * DYN_STRIDE];
  constexpr int NB = nb_of<CL>();
  const int n = D.n, e0 = blockIdx.x * DYN_TILE, ne = min(DYN_TILE, n - e0);
  if ((int)threadIdx.x < ne) {
    const int e = e0 + threadIdx.x;
    float* L = lds + threadIdx.x * DYN_STRIDE;
    EnvState S;
    load_state(D.st, n, e, S);
    M3 E[BEZ_NL]; V3 r[BEZ_NL]; SV V[BEZ_NL];
    link_frames<CL, false>(S, D.flags, E, r, V);
    dyn_joint_words(L, E, r);
    static_for<NB>([&](auto I) {
      const BodyFrame f = body_frame<CL>(decltype(I)::value);
      dyn_put3(L, DYN_XB + 3 * decltype(I)::value, r[f.link] + mul(E[f.link], f.off));
    });
    if (M) dyn_mass_words<CL>(D, e, L, E, r);
  }
  __syncthreads();
  if (J) {
    float4* out = reinterpret_cast<float4*>(J + (size_t)e0 * NB * 6 * DYN_NG);
    const int total = ne * NB * 6 * (DYN_NG / 4);
    for (int i = threadIdx.x; i < total; i += DYN_THREADS) {
      const int c4 = i % (DYN_NG / 4), t = i / (DYN_NG / 4), row = t % 6, b = (t / 6) % NB, el = t / (6 * NB);
      const float* L = lds + el * DYN_STRIDE;
      const uint32_t mask = BODY_ANCESTORS<CL>.m[b];
      const V3 x = lds3(L + DYN_XB + 3 * b);
      out[i] = make_float4(jacobian_entry(L, mask, x, row, 4 * c4), jacobian_entry(L, mask, x, row, 4 * c4 + 1),
                           jacobian_entry(L, mask, x, row, 4 * c4 + 2), jacobian_entry(L, mask, x, row, 4 * c4 + 3));
    }
  }
  if (M) {
    float4* out = reinterpret_cast<float4*>(M + (size_t)e0 * DYN_NG * DYN_NG);
    constexpr int PER_ENV = DYN_NG * DYN_NG / 4;
    for (int i = threadIdx.x; i < ne * PER_ENV; i += DYN_THREADS) {
      const float* Ms = lds + (i / PER_ENV) * DYN_STRIDE + DYN_MS;
      const int16_t* sl = MASS_SLOTS.s + 4 * (i % PER_ENV);
      out[i] = make_float4(Ms[sl[0]], Ms[sl[1]], Ms[sl[2]], Ms[sl[3]]);
    }
  }
}

// ---- bez_sim_inverse_dynamics (definition: include/bez_sim.h "Inverse dynamics"): recursive Newton-Euler in the frame every bias force
// here uses (world axes about the root origin), where a subtree's wrench is the plain sum of its links' wrenches.
// A workgroup is ONE wave and takes ID_TILE consecutive envs.  All lanes bring the tile's udot rows -- one contiguous range -- into LDS
// (tile_load_or_zero); then one lane per env walks the tree CHAIN BY CHAIN (for_each_chain): out along a chain (two legs of 6 joints,
// two arms and the head of 2) keeping per joint only S = [a; r x a] and handing the link's acceleration down, back along it adding up the wrenches and emitting
// tau = S . F into the udot slot it has just consumed, and the chain's total joins the torso's wrench.  At most six links are live,
// never the 19 frames of link_frames.  Last, all lanes write the tile's rows as one contiguous range of float4 stores.
// A term is dropped by zeroing its input (udot, the velocities, g): one code path, and the dropped term's products are exact zeros.
// The chains are taken last to first and each is summed from its leaf, the order in which refresh_dynamics_kernel adds up the masses.
constexpr int ID_TILE = 16, ID_THREADS = 64, ID_STRIDE = DYN_NG + 1;   // odd row stride: the lanes' own rows start in distinct LDS banks
// One link of a chain and, by recursion, the links below it: on the way out the link's frame, velocity and accelerations from its
// parent's (by value: each level keeps its own) and its own wrenches; on the way back tau = S . F goes to U[5 + L], the slot whose udot
// the way out consumed, and the subtree's wrenches are returned.  (Plain locals per level, no arrays over the links: the compiler keeps
// arrays of spatial vectors live as whole register blocks for all five chains at once.)
// The three terms are carried APART -- the acceleration as aI (from udot) and aV (velocity products), the wrench as i = I aI,
// v = I aV + v x* I v and g = -I [0; g] -- and meet only in the last two additions of every output element: the wrenches that cancel
// along a chain to a small joint torque are then rounded within their own term, a term's value does not depend on which other terms
// were asked for, and all terms together are the fp32 sum (inertia + velocity) + gravity of the three single-term results.
struct IdCtx { const DynArgs& D; int e; bool vel; float quirk_z; V3 g; };
struct IdWrench { SV i, v, g; };
BEZ_DEV IdWrench operator+(const IdWrench& a, const IdWrench& b) { return {a.i + b.i, a.v + b.v, a.g + b.g}; }
BEZ_DEV IdWrench id_wrench(const LinkInertia& I, SV aI, SV aV, SV pV, V3 g) {
  return {inertia_times(I, aI), inertia_times(I, aV) + pV, mksv(-cross(I.h, g), -(g * I.m))};
}
BEZ_DEV float id_sum(float i, float v, float g) { return (i + v) + g; }
template <int L, int END, bool CL>
BEZ_DEV IdWrench id_links(const IdCtx& C, M3 E, V3 r, SV V, SV aI, SV aV, float* U) {
  const float q = state_at(C.D, F_Q + L - 1, C.e), qd = C.vel ? state_at(C.D, F_QD + L - 1, C.e) : 0.f, qdd = U[5 + L];
  SV S, cb;
  link_kinematics<L>(q, qd, E, r, V, S, cb, C.quirk_z);
  aI = aI + S * qdd; aV = aV + cb;
  LinkInertia LI; SV pV;
  link_inertia<L, CL>(mass_scale_of(C.D, C.e, L), mk(0, 0, 0), E, r, V, LI, pV);
  IdWrench F = id_wrench(LI, aI, aV, pV, C.g);
  if constexpr (L + 1 < END) F = F + id_links<L + 1, END, CL>(C, E, r, V, aI, aV, U);
  U[5 + L] = id_sum(fmaf(C.D.armature, qdd, dot(S, F.i)), dot(S, F.v), dot(S, F.g));
  return F;
}
template <bool CL>
__global__ void __launch_bounds__(ID_THREADS) inverse_dynamics_kernel(DynArgs D, const float* __restrict__ udot, float* __restrict__ out, uint32_t terms) {
  __shared__ float rows[ID_TILE * ID_STRIDE];
  const int n = D.n, e0 = blockIdx.x * ID_TILE, ne = min(ID_TILE, n - e0);
  tile_load_or_zero<DYN_NG, ID_STRIDE, ID_THREADS>(rows, (udot && (terms & BEZ_ID_INERTIA)) ? udot + (size_t)e0 * DYN_NG : nullptr, ne);
  __syncthreads();
  if ((int)threadIdx.x < ne) {
    const int e = e0 + threadIdx.x;
    float* U = rows + threadIdx.x * ID_STRIDE;
    const bool vel = (terms & BEZ_ID_VELOCITY) != 0;
    const M3 E0 = root_rotation(D, e);
    const SV V0 = vel ? mksv(state3_at(D, F_ROOT_ANG, e), state3_at(D, F_ROOT_LIN, e)) : svzero();
    V3 g = mk(0, 0, 0);
    if (terms & BEZ_ID_GRAVITY) g = gravity_of(D, e);
    // spatial acceleration of the torso about the (momentarily fixed) point its origin passes through: [wdot; vdot - w x v]
    const SV aI0 = mksv(mk(U[3], U[4], U[5]), mk(U[0], U[1], U[2])), aV0 = mksv(mk(0, 0, 0), -cross(V0.a, V0.l));
    LinkInertia I0; SV pV0;
    link_inertia<0, CL>(mass_scale_of(D, e, 0), mk(0, 0, 0), E0, mk(0, 0, 0), V0, I0, pV0);
    IdWrench F0 = id_wrench(I0, aI0, aV0, pV0, g);
    // (the env index is made opaque per chain, together with the wrench so far: otherwise every chain's loads are issued up front and
    // the five chains are interleaved, at the price of their registers)
    IdCtx C = {D, e, vel, quirk_rz<CL>(D.flags), g};
    for_each_chain<true>([&](auto first, auto len) {
      constexpr int FIRST = decltype(first)::value, LEN = decltype(len)::value;
      asm volatile("" : "+v"(C.e), "+v"(F0.i.l.x));
      F0 = F0 + id_links<FIRST, FIRST + LEN, CL>(C, E0, mk(0, 0, 0), V0, aI0, aV0, U);
    });
    U[0] = id_sum(F0.i.l.x, F0.v.l.x, F0.g.l.x); U[1] = id_sum(F0.i.l.y, F0.v.l.y, F0.g.l.y); U[2] = id_sum(F0.i.l.z, F0.v.l.z, F0.g.l.z);
    U[3] = id_sum(F0.i.a.x, F0.v.a.x, F0.g.a.x); U[4] = id_sum(F0.i.a.y, F0.v.a.y, F0.g.a.y); U[5] = id_sum(F0.i.a.z, F0.v.a.z, F0.g.a.z);
  }
  __syncthreads();
  tile_store<DYN_NG, ID_STRIDE, ID_THREADS>(rows, out + (size_t)e0 * DYN_NG, ne);
}

// ---- bez_sim_centroidal (definition: include/bez_sim.h "Centroidal dynamics"): the composite-rigid-body sums of refresh_dynamics_kernel
// stopped at rows 0:6 of M -- no path-pair products -- with the moment shifted from the root origin to the centre of mass.
// A workgroup is ONE wave and takes CM_TILE consecutive envs.  Phase 1, one lane per env, in world axes about the root origin (where the
// LinkInertia composites add up without transforms): forward kinematics with velocities, the links' inertias, then links 18 -> 1: F_l =
// I^c_l S_l as [lin; ang] -- column 6 + l - 1 of the momentum map about the root origin -- goes to the env's LDS row where A_G has it, and
// the composite joins its parent's.  With I^c_0 = {m, h, Ibar} the centre of mass is c = h / m; a second pass over the columns takes
// c x (linear rows) off the angular rows and adds up the momentum A_G u on the way.  The base block is written from its definition:
// m I, -skew(h), the constant 0 and I_G = Ibar - m (|c|^2 I - c c^T), six values for nine slots.
// The kinetic energy is the sum over links of 1/2 V_l . I_l V_l with the link's OWN inertia and spatial velocity (+ 1/2 armature |qd|^2):
// 19 non-negative terms, equal to 1/2 u^T M u, without the subtree sums that the rows 6:24 of M u would need.
// Phase 2, all lanes: the tile's rows are two contiguous ranges (CM_TILE x 16 floats of state, CM_TILE x 144 of matrix), stored as float4
// (pointers that are not 16-byte aligned: a scalar path to the same bits).  Rows of CM_STRIDE words, odd: the lanes of phase 1 write
// distinct banks.
constexpr int CM_TILE = 16, CM_THREADS = 64, CM_MATRIX = 6 * DYN_NG, CM_STRIDE = (BEZ_CM_WORDS + CM_MATRIX) | 1;
template <bool CL>
__global__ void __launch_bounds__(CM_THREADS) centroidal_kernel(DynArgs D, float* __restrict__ state_out, float* __restrict__ matrix_out) {
  __shared__ float lds[CM_TILE * CM_STRIDE];
  const int n = D.n, e0 = blockIdx.x * CM_TILE, ne = min(CM_TILE, n - e0);
  if ((int)threadIdx.x < ne) {
    const int e = e0 + threadIdx.x;
    float* W = lds + threadIdx.x * CM_STRIDE;   // the env's state words
    float* A = W + BEZ_CM_WORDS;                // its A_G, 6 x 24 row-major
    auto put_col = [&](int row0, int c, V3 v) { A[row0 * DYN_NG + c] = v.x; A[(row0 + 1) * DYN_NG + c] = v.y; A[(row0 + 2) * DYN_NG + c] = v.z; };
    auto get_col = [&](int row0, int c) { return mk(A[row0 * DYN_NG + c], A[(row0 + 1) * DYN_NG + c], A[(row0 + 2) * DYN_NG + c]); };
    EnvState S;
    load_state(D.st, n, e, S);
    M3 E[BEZ_NL]; V3 r[BEZ_NL]; SV V[BEZ_NL];
    link_frames<CL, true>(S, D.flags, E, r, V);
    LinkInertia Ic[BEZ_NL];
    float ke2 = 0.f;   // twice the kinetic energy
    link_inertias<CL>(D, e, E, r, Ic, [&](auto I) { constexpr int l = decltype(I)::value; ke2 += dot(V[l], inertia_times(Ic[l], V[l])); });
    float qd2 = 0.f;
    composite_sweep(Ic, E, r, [&](auto Lk, SV F) {
      constexpr int l = decltype(Lk)::value;
      put_col(0, 5 + l, F.l);
      put_col(3, 5 + l, F.a);
      qd2 = fmaf(S.qd[l - 1], S.qd[l - 1], qd2);
    });
    const LinkInertia& C = Ic[0];
    const float m = C.m;
    const V3 h = C.h, c = mk(h.x / m, h.y / m, h.z / m), w = S.root_ang;
    Sym3 G;   // I_G = Ibar - m (|c|^2 I - c c^T): each of the six values is formed once and written to both triangles
    G.xx = C.Ibar.xx - fmaf(h.y, c.y, h.z * c.z); G.yy = C.Ibar.yy - fmaf(h.x, c.x, h.z * c.z); G.zz = C.Ibar.zz - fmaf(h.x, c.x, h.y * c.y);
    G.xy = fmaf(h.x, c.y, C.Ibar.xy); G.xz = fmaf(h.x, c.z, C.Ibar.xz); G.yz = fmaf(h.y, c.z, C.Ibar.yz);
    put_col(0, 0, mk(m, 0.f, 0.f)); put_col(0, 1, mk(0.f, m, 0.f)); put_col(0, 2, mk(0.f, 0.f, m));
    put_col(0, 3, mk(0.f, -h.z, h.y)); put_col(0, 4, mk(h.z, 0.f, -h.x)); put_col(0, 5, mk(-h.y, h.x, 0.f));   // -skew(h) = -m skew(c)
    put_col(3, 0, mk(0, 0, 0)); put_col(3, 1, mk(0, 0, 0)); put_col(3, 2, mk(0, 0, 0));
    put_col(3, 3, mk(G.xx, G.xy, G.xz)); put_col(3, 4, mk(G.xy, G.yy, G.yz)); put_col(3, 5, mk(G.xz, G.yz, G.zz));
    // the momentum A_G u: the base columns (their structural zeros skipped), then the joints'
    V3 P = S.root_lin * m - cross(h, w), L = mul(G, w);
    static_for<BEZ_ND>([&](auto I) {
      constexpr int d = decltype(I)::value;
      const V3 Fl = get_col(0, 6 + d), Fg = get_col(3, 6 + d) - cross(c, Fl);
      put_col(3, 6 + d, Fg);
      P = fma3(Fl, S.qd[d], P);
      L = fma3(Fg, S.qd[d], L);
    });
    const V3 g = gravity_of(D, e), com = S.root_pos + c;
    W[BEZ_CM_COM] = com.x; W[BEZ_CM_COM + 1] = com.y; W[BEZ_CM_COM + 2] = com.z;
    // (x + 0.0f is x except that it turns -0.0 into +0.0: a state at rest and a zero gravity row give zeros to the bit)
    P = P + mk(0.f, 0.f, 0.f); L = L + mk(0.f, 0.f, 0.f);
    W[BEZ_CM_COM_VEL] = P.x / m; W[BEZ_CM_COM_VEL + 1] = P.y / m; W[BEZ_CM_COM_VEL + 2] = P.z / m;
    W[BEZ_CM_LIN_MOM] = P.x; W[BEZ_CM_LIN_MOM + 1] = P.y; W[BEZ_CM_LIN_MOM + 2] = P.z;
    W[BEZ_CM_ANG_MOM] = L.x; W[BEZ_CM_ANG_MOM + 1] = L.y; W[BEZ_CM_ANG_MOM + 2] = L.z;
    W[BEZ_CM_MASS] = m;
    W[BEZ_CM_KINETIC] = 0.5f * fmaf(D.armature, qd2, ke2) + 0.f;
    W[BEZ_CM_POTENTIAL] = 0.f - m * dot(g, com);
    W[15] = 0.f;
  }
  __syncthreads();
  if (state_out) tile_store<BEZ_CM_WORDS, CM_STRIDE, CM_THREADS>(lds, state_out + (size_t)e0 * BEZ_CM_WORDS, ne);
  if (matrix_out) tile_store<CM_MATRIX, CM_STRIDE, CM_THREADS>(lds + BEZ_CM_WORDS, matrix_out + (size_t)e0 * CM_MATRIX, ne);
}

// ---- bez_sim_body_accelerations (definition: include/bez_sim.h "Body accelerations"): the outward half of inverse_dynamics_kernel -- no
// inertias, no return sweep -- with a read-out per body like refresh_rigid_body_kernel's.
// A workgroup is ONE wave and takes ACC_TILE consecutive envs.  All lanes bring the tile's udot rows into LDS (tile_load_or_zero); then one
// lane per env walks the tree chain by chain, in world axes about the root origin, carrying per link only its frame E, r, its spatial
// velocity V and its spatial acceleration in two parts: aI (from udot: aI += S qdd) and aV (velocity products: aV += cb of
// link_kinematics).  Every body on the link is read out where the walk stands: with x the body's origin relative to the root origin,
//     UDOT      [aI.l + aI.a x x ; aI.a]
//     VELOCITY  [aV.l + aV.a x x + w x (v + w x x) ; aV.a]        (classical acceleration of the origin: d/dt of RIGID_BODY_STATE[7:10])
//     GRAVITY   [0 - g ; 0]
// and the element is (UDOT + VELOCITY) + GRAVITY, the parts canonicalised (x + 0.0f: -0.0 becomes +0.0) so that a dropped or vanishing
// term is +0.0f to the bit.  BEZ_SPACE_LOCAL turns both triples by the link frame's transpose after that sum.
// The velocity part is evaluated with root_lin = 0: J's columns 0:3 are constant, so Jdot u does not depend on root_lin (a uniform
// translation changes no acceleration), and with it go the pair -w x v + w x v that would cancel in every row and the torso's aV, which
// is then zero by construction.  Bodies of the torso link take their rows from the definition: [vdot + wdot x x ; wdot] and
// [w x (w x x) ; 0], so the torso itself (x = 0) returns udot[0:6] and zeros.
// Last, all lanes write the tile's rows -- one contiguous range of ne x 6 NB floats, not whole float4s -- with tile_store.
constexpr int ACC_TILE = 16, ACC_THREADS = 64, ACC_USTRIDE = DYN_NG + 1;   // odd row strides: the lanes' own rows start in distinct LDS banks
struct AccCtx { float* O; V3 g; bool local; };   // the env's output row in LDS, 0 - g, BEZ_SPACE_LOCAL
BEZ_DEV V3 acc_sum(V3 i, V3 v, V3 g) {
  const V3 z = mk(0.f, 0.f, 0.f);
  return ((i + z) + (v + z)) + g;
}
// the rows of every body fixed to link L; E, r, V, aI, aV: the link's
template <bool CL, int L>
BEZ_DEV void acc_bodies(const AccCtx& C, const M3& E, V3 r, SV V, SV aI, SV aV) {
  for_each_body_of_link<CL, L>([&](auto B, const BodyFrame& bf, bool at_link_origin) {
    const V3 x = at_link_origin ? r : r + mul(E, bf.off);
    V3 li, lv;
    if constexpr (L == 0) {
      li = at_link_origin ? aI.l : aI.l + cross(aI.a, x);
      lv = at_link_origin ? mk(0.f, 0.f, 0.f) : cross(V.a, cross(V.a, x));
    } else {
      li = point_of(aI, x);
      lv = point_of(aV, x) + cross(V.a, point_of(V, x));
    }
    V3 lin = acc_sum(li, lv, C.g), ang = acc_sum(aI.a, aV.a, mk(0.f, 0.f, 0.f));
    if (C.local) { lin = mulT(E, lin) + mk(0.f, 0.f, 0.f); ang = mulT(E, ang) + mk(0.f, 0.f, 0.f); }   // (products of +0.0 may be -0.0)
    float* O = C.O + 6 * decltype(B)::value;
    O[0] = lin.x; O[1] = lin.y; O[2] = lin.z; O[3] = ang.x; O[4] = ang.y; O[5] = ang.z;
  });
}
template <bool CL>
__global__ void __launch_bounds__(ACC_THREADS) body_accelerations_kernel(DynArgs D, const float* __restrict__ udot, float* __restrict__ out,
                                                                         uint32_t terms, int local) {
  constexpr int WIDTH = 6 * nb_of<CL>(), STRIDE = WIDTH | 1;
  __shared__ float urows[ACC_TILE * ACC_USTRIDE];
  __shared__ float orows[ACC_TILE * STRIDE];
  const int n = D.n, e0 = blockIdx.x * ACC_TILE, ne = min(ACC_TILE, n - e0);
  tile_load_or_zero<DYN_NG, ACC_USTRIDE, ACC_THREADS>(urows, (udot && (terms & BEZ_ACC_UDOT)) ? udot + (size_t)e0 * DYN_NG : nullptr, ne);
  __syncthreads();
  if ((int)threadIdx.x < ne) {
    int e = e0 + threadIdx.x;
    const float* U = urows + threadIdx.x * ACC_USTRIDE;
    const bool vel = (terms & BEZ_ACC_VELOCITY) != 0;
    const M3 E0 = root_rotation(D, e);
    const SV V0 = mksv(vel ? state3_at(D, F_ROOT_ANG, e) : mk(0.f, 0.f, 0.f), mk(0.f, 0.f, 0.f));
    // spatial acceleration of the torso about the (momentarily fixed) point its origin passes through: [wdot; vdot - w x v], whose
    // second part is a velocity product that vanishes with root_lin = 0
    const SV aI0 = mksv(mk(U[3], U[4], U[5]), mk(U[0], U[1], U[2]));
    V3 g = mk(0.f, 0.f, 0.f);
    if (terms & BEZ_ACC_GRAVITY) g = gravity_of(D, e);
    AccCtx C = {orows + threadIdx.x * STRIDE, mk(0.f - g.x, 0.f - g.y, 0.f - g.z), local != 0};
    const float quirk_z = quirk_rz<CL>(D.flags);
    acc_bodies<CL, 0>(C, E0, mk(0.f, 0.f, 0.f), V0, aI0, svzero());
    for_each_chain<false>([&](auto first, auto len) {
      constexpr int FIRST = decltype(first)::value, LEN = decltype(len)::value;
      asm volatile("" : "+v"(e));   // (opaque per chain: otherwise every chain's loads are issued up front, at the price of their registers)
      M3 E = E0; V3 r = mk(0.f, 0.f, 0.f); SV V = V0, aI = aI0, aV = svzero();
      static_for<LEN>([&](auto I) {
        constexpr int L = FIRST + decltype(I)::value;
        SV S, cb;
        link_kinematics<L>(state_at(D, F_Q + L - 1, e), vel ? state_at(D, F_QD + L - 1, e) : 0.f, E, r, V, S, cb, quirk_z);
        aI = aI + S * U[5 + L]; aV = aV + cb;
        acc_bodies<CL, L>(C, E, r, V, aI, aV);
      });
    });
  }
  __syncthreads();
  tile_store<WIDTH, STRIDE, ACC_THREADS>(orows, out + (size_t)e0 * WIDTH, ne);
}

// ---- bez_sim_generalized_forces (definition: include/bez_sim.h "Generalised forces"): sum_b J_b^T w_b without J -- the return sweep of
// inverse_dynamics_kernel with the links' inertial wrenches replaced by the wrenches the caller hands in.
// A workgroup is ONE wave and takes GF_TILE consecutive envs.  All lanes bring the tile's force, torque and position rows -- per tensor
// one contiguous range of ne x 3 B floats, B with the ball's row where the task has one, not whole float4s -- into LDS with
// tile_load; then one lane per env walks the tree chain by chain in link-local coordinates: out along a chain for each link's
// frame E, r in the root's axes (link_kinematics with qd = 0; ENV inputs are turned by it, LOCAL inputs need no turn), collecting the
// wrenches of the bodies fixed to the link as [t + d x f ; f] in the link's axes, d the point of application relative to the link's
// origin; back along it adding up the subtree's wrench, writing tau = +-M[axis] to the env's output row in LDS and taking the wrench to
// the parent's axes and origin; the chain's total, by then in the root's axes about the root origin, joins the torso's wrench, which is
// turned to world axes for rows 0:6 (ENV wrenches on the torso's own bodies stay in world axes throughout).  A body whose
// force and torque rows are all zero is skipped before its position row is looked at (ext_prepare_kernel's rule: a NaN is != 0 and goes
// in); the ball's row is never read.  Every output is canonicalised (x + 0.0f), so a subtree without a loaded body gives +0.0f to the bit.
// Last, all lanes write the tile's (ne, 24) rows with tile_store.
constexpr int GF_TILE = 16, GF_THREADS = 64, GF_OSTRIDE = DYN_NG + 1;   // odd row strides: the lanes' own rows start in distinct LDS banks
// the env's rows in LDS (null: the tensor was not given), its root position, the call's space, and the rotation whose transpose takes
// an ENV vector into the root's axes
struct GfCtx { const float *F, *T, *X; V3 root_pos; bool local, at_origin; M3 Rin; };
// the wrench [moment about the LINK's origin; force], in the LINK's own axes, of every loaded body fixed to link L; E, r: the link's
// frame in the root's axes, which only ENV inputs need -- a LOCAL row is used as it is given
template <bool CL, int L>
BEZ_DEV SV gf_bodies(const GfCtx& C, const M3& E, V3 r) {
  SV W = svzero();
  for_each_body_of_link<CL, L>([&](auto B, const BodyFrame& bf, bool at_link_origin) {
    constexpr int b = decltype(B)::value;
    const V3 f = C.F ? lds3(C.F + 3 * b) : mk(0.f, 0.f, 0.f), t = C.T ? lds3(C.T + 3 * b) : mk(0.f, 0.f, 0.f);
    if (f.x != 0.f || f.y != 0.f || f.z != 0.f || t.x != 0.f || t.y != 0.f || t.z != 0.f) {   // (a NaN is != 0: it goes in)
      const V3 fl = C.local ? f : mulT(E, mulT(C.Rin, f)), tl = C.local ? t : mulT(E, mulT(C.Rin, t));
      V3 d;   // the point of application relative to the link's origin
      if (!C.X) d = C.at_origin ? bf.off : bf.off + bf.com;
      else if (C.local) d = bf.off + lds3(C.X + 3 * b);
      else d = mulT(E, mulT(C.Rin, lds3(C.X + 3 * b) - C.root_pos) - r);
      W = W + mksv((!C.X && C.at_origin && at_link_origin) ? tl : tl + cross(d, fl), fl);
    }
  });
  return W;
}
// v in link L's axes -> in its parent's: the joint's rotation about the frame axis it leaves alone (rotate_about's matrix)
template <int L>
BEZ_DEV V3 gf_to_parent(V3 v, float s, float c) {
  constexpr int ax = axis_index(L);
  if constexpr (ax == 0) return mk(v.x, fmaf(c, v.y, -(s * v.z)), fmaf(s, v.y, c * v.z));
  else if constexpr (ax == 1) return mk(fmaf(s, v.z, c * v.x), v.y, fmaf(c, v.z, -(s * v.x)));
  else return mk(fmaf(c, v.x, -(s * v.y)), fmaf(s, v.x, c * v.y), v.z);
}
// One link of a chain and, by recursion, the links below it (id_links without inertias), in LINK-LOCAL coordinates: the subtree's
// wrench is kept in the link's own axes about its own origin, where the joint torque is one component of the moment, tau = +-M[axis],
// and goes up to the parent by the joint's rotation and the constant joint origin.  The definition works per link: a LOCAL wrench gives
// joint torques that do not depend on the root pose, and no product of six rotations stands between a LOCAL row and its own joint.
// Measured on MI355X against the bar of a yardstick that works per link (tests/test_gpu_generalized_forces.py), the joint rows of
// three world-axes forms of this walk reach: about the root origin (id_links' frame; a foot's joint torque is then the difference of
// two moments of 0.3 m x 10 N that cancel to 0.05 m x 10 N) 1.09; about the links' origins in world axes (E0^T E0 - I of an fp32
// quaternion, unit to 1e-7, enters every LOCAL row) 1.23; about the links' origins in the root's axes (the rounding of the accumulated
// link rotation is left) 1.10.  Returns the subtree's wrench in the PARENT's axes about the parent's origin; Q: the env's output row.
template <int L, int END, bool CL>
BEZ_DEV SV gf_links(const GfCtx& C, const DynArgs& D, int e, float quirk_z, M3 E, V3 r, float* Q) {
  const float q = state_at(D, F_Q + L - 1, e);
  SV S, cb, V = svzero();
  link_kinematics<L>(q, 0.f, E, r, V, S, cb, quirk_z);
  SV F = gf_bodies<CL, L>(C, E, r);
  if constexpr (L + 1 < END) F = F + gf_links<L + 1, END, CL>(C, D, e, quirk_z, E, r, Q);
  Q[5 + L] = axis_sign(L) * pick(F.a, axis_index(L)) + 0.f;
  float sn, cs;
  fsincos(axis_sign(L) * q, &sn, &cs);
  const V3 xyz = mk((float)BEZ_LINK_XYZ[L][0], (float)BEZ_LINK_XYZ[L][1], L == BEZ_BOXCL_LINK ? quirk_z : (float)BEZ_LINK_XYZ[L][2]);
  const V3 fp = gf_to_parent<L>(F.l, sn, cs);
  return mksv(gf_to_parent<L>(F.a, sn, cs) + cross(xyz, fp), fp);
}
template <bool CL>
__global__ void __launch_bounds__(GF_THREADS) generalized_forces_kernel(DynArgs D, const float* __restrict__ forces, const float* __restrict__ torques,
                                                                        const float* __restrict__ positions, int space, int has_ball,
                                                                        float* __restrict__ out) {
  constexpr int NB = nb_of<CL>(), STRIDE = (3 * (NB + 1)) | 1;
  __shared__ float in_rows[3][GF_TILE * STRIDE];
  __shared__ float orows[GF_TILE * GF_OSTRIDE];
  const int n = D.n, e0 = blockIdx.x * GF_TILE, ne = min(GF_TILE, n - e0);
  const float* in[3] = {forces, torques, positions};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (!in[k]) continue;
    if (has_ball) tile_load<3 * (NB + 1), STRIDE, GF_THREADS>(in_rows[k], in[k] + (size_t)e0 * (3 * (NB + 1)), ne);
    else tile_load<3 * NB, STRIDE, GF_THREADS>(in_rows[k], in[k] + (size_t)e0 * (3 * NB), ne);
  }
  __syncthreads();
  if ((int)threadIdx.x < ne) {
    int e = e0 + threadIdx.x;
    float* Q = orows + threadIdx.x * GF_OSTRIDE;
    auto row = [&](int k) -> const float* { return in[k] ? in_rows[k] + threadIdx.x * STRIDE : nullptr; };
    const M3 E0 = root_rotation(D, e);
    const M3 I3 = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    const V3 O = mk(0.f, 0.f, 0.f);
    const GfCtx C = {row(0), row(1), row(2), state3_at(D, F_ROOT_POS, e), (space & BEZ_SPACE_LOCAL) != 0, (space & BEZ_GF_AT_ORIGIN) != 0, E0};
    const float quirk_z = quirk_rz<CL>(D.flags);
    // the torso's bodies: in the root's axes like the chains' totals, except ENV wrenches at ENV points, which stay in world axes,
    // untouched by E0 (a wrench on body 0 at the root position comes out as it went in)
    SV Fw = svzero(), F0 = svzero();
    if (C.local || !C.X) F0 = gf_bodies<CL, 0>(C, I3, O);
    else {
      GfCtx Cw = C;
      Cw.Rin = I3;
      Fw = gf_bodies<CL, 0>(Cw, I3, O);
    }
    for_each_chain<true>([&](auto first, auto len) {
      constexpr int FIRST = decltype(first)::value, LEN = decltype(len)::value;
      asm volatile("" : "+v"(e), "+v"(F0.l.x));   // (opaque per chain, as in inverse_dynamics_kernel)
      F0 = F0 + gf_links<FIRST, FIRST + LEN, CL>(C, D, e, quirk_z, I3, O, Q);
    });
    const V3 fo = Fw.l + mul(E0, F0.l), mo = Fw.a + mul(E0, F0.a);   // the root-frame total, turned to world axes
    Q[0] = fo.x + 0.f; Q[1] = fo.y + 0.f; Q[2] = fo.z + 0.f;
    Q[3] = mo.x + 0.f; Q[4] = mo.y + 0.f; Q[5] = mo.z + 0.f;
  }
  __syncthreads();
  tile_store<DYN_NG, GF_OSTRIDE, GF_THREADS>(orows, out + (size_t)e0 * DYN_NG, ne);
}

// ---- bez_sim_limb_ik (definition: include/bez_sim.h "Limb inverse kinematics"): damped least squares on each of the five chains off
// the torso, whose joints are disjoint: five independent problems of 2, 2, 6, 2, 6 unknowns per env.
// A workgroup takes IK_TILE consecutive envs.  All lanes bring the tile's (ne, 35) target rows -- one contiguous range -- into LDS
// (tile_load).  The workgroup is five waves, and wave c takes chain c of every env of the tile: one lane per (env, chain), with
// every wave running one chain's code (the links are compile-time: lanes of one wave on different chains would run the five bodies
// one after the other).  The family's form -- one wave, one lane per env walking the five chains in turn -- computes the same bits and
// was measured on MI355X at 4096 envs, 8 iterations: 56.6 us against this form's 19.3 us (profiles/limb_ik_tiles.txt).
// Per chain and iteration, in the root's axes about the root origin: still_chain_walk down the chain keeping each joint's axis and
// origin, the tip's pose error, the k columns [a x (p - r); a], the lower triangle of J^T W J + lambda^2 I, its Cholesky factor and the
// two substitutions -- all over compile-time indices, so every array lives in registers; only the iteration count is a run-time loop.
// The angles and the errors go to the env's rows in LDS, and all lanes write the tile's (ne, 18) and (ne, 30) rows with
// tile_store.  The limit rows come as two pointers beside DynArgs, not inside it: DynArgs heads every neighbour's arguments, and
// growing it would move theirs.
constexpr int IK_TILE = 32, IK_THREADS = 64 * BEZ_IK_CHAINS, IK_TW = 7 * BEZ_IK_CHAINS, IK_EW = 6 * BEZ_IK_CHAINS;
constexpr int IK_TSTRIDE = IK_TW | 1, IK_QSTRIDE = BEZ_ND | 1, IK_ESTRIDE = IK_EW | 1;   // odd row strides: the lanes' own rows start in distinct LDS banks
static_assert(IK_TILE <= 64, "one lane of a wave per env of the tile");
// The Cholesky factorisation of a symmetric positive definite K x K matrix given by its lower triangle, in place as L L^T with the
// reciprocals of L's diagonal beside it, and the two substitutions that solve L L^T x = b in place.  Every index is compile-time, so
// the factor lives in registers.  Shared with forward_dynamics_kernel.
template <int K>
BEZ_DEV void chol_factor(float (&A)[K][K], float (&inv)[K]) {
#pragma unroll
  for (int j = 0; j < K; ++j) {
    float d = A[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d = fmaf(-A[j][k], A[j][k], d);
    d = sqrtf(d);
    inv[j] = 1.f / d;
#pragma unroll
    for (int i = j + 1; i < K; ++i) {
      float s = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) s = fmaf(-A[i][k], A[j][k], s);
      A[i][j] = s * inv[j];
    }
  }
}
template <int K>
BEZ_DEV void chol_solve(const float (&A)[K][K], const float (&inv)[K], float (&x)[K]) {
#pragma unroll
  for (int i = 0; i < K; ++i) {
#pragma unroll
    for (int k = 0; k < i; ++k) x[i] = fmaf(-A[i][k], x[k], x[i]);
    x[i] *= inv[i];
  }
#pragma unroll
  for (int i = K - 1; i >= 0; --i) {
#pragma unroll
    for (int k = i + 1; k < K; ++k) x[i] = fmaf(-A[k][i], x[k], x[i]);
    x[i] *= inv[i];
  }
}
// what a chain needs of the call: the env, the joint limit rows, the root pose that takes ENV targets into the root's frame
struct IkCtx { const DynArgs& D; const float *lower, *upper; int e; float quirk_z; bool env; M3 E0; V3 root_pos; float lam2, max_step; int iters; };
// x held to [lo, hi]; a NaN stays a NaN (fminf / fmaxf would return the limit)
BEZ_DEV float ik_clamp(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }
// T: the chain's target row (7 words), Q: the env's angle row (18), R: the chain's error row (6), all in LDS
template <bool CL, int C>
BEZ_DEV void ik_chain(const IkCtx& K, const BezIkParams& P, const float* T, float* Q, float* R) {
  constexpr int FIRST = chain_first(C), LEN = chain_len(C), D0 = FIRST - 1;
  float q[LEN];
#pragma unroll
  for (int i = 0; i < LEN; ++i) q[i] = state_at(K.D, F_Q + D0 + i, K.e);
  const float wp = P.weight[C][0], wr = P.weight[C][1];
  if (wp == 0.f && wr == 0.f) {   // not asked for: the state's angles, and the target row is not looked at
#pragma unroll
    for (int i = 0; i < LEN; ++i) Q[D0 + i] = q[i];
#pragma unroll
    for (int k = 0; k < 6; ++k) R[k] = 0.f;
    return;
  }
  float lo[LEN], hi[LEN];
#pragma unroll
  for (int i = 0; i < LEN; ++i) {
    lo[i] = K.lower ? K.lower[(size_t)K.e * BEZ_ND + D0 + i] : (float)BEZ_DOF_LOWER[D0 + i];
    hi[i] = K.upper ? K.upper[(size_t)K.e * BEZ_ND + D0 + i] : (float)BEZ_DOF_UPPER[D0 + i];
  }
  // the target in the root's frame
  V3 pd = mk(T[0], T[1], T[2]);
  const float nq = 1.f / sqrtf(fmaf(T[3], T[3], fmaf(T[4], T[4], fmaf(T[5], T[5], T[6] * T[6]))));
  M3 Rd = quat_to_mat(T[3] * nq, T[4] * nq, T[5] * nq, T[6] * nq);
  if (K.env) {
    pd = mulT(K.E0, pd - K.root_pos);
    const V3 c0 = mulT(K.E0, col(Rd, 0)), c1 = mulT(K.E0, col(Rd, 1)), c2 = mulT(K.E0, col(Rd, 2));
    set_col(Rd, 0, c0); set_col(Rd, 1, c1); set_col(Rd, 2, c2);
  }
  // the controlled point in the last link's frame: the end body's origin displaced by the caller's offset
  const BodyFrame bf = body_frame<CL>(link_body<CL>(FIRST + LEN - 1));
  const V3 tip = bf.off + mk(P.offset[C][0], P.offset[C][1], P.offset[C][2]);
  V3 ep, er;
  for (int it = 0;; ++it) {
    M3 E = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    V3 r = mk(0.f, 0.f, 0.f), a[LEN], ro[LEN];
    still_chain_walk<FIRST, LEN>(E, r, K.quirk_z, [&](auto L) { return q[decltype(L)::value - FIRST]; }, [&](auto L, const SV& S) {
      a[decltype(L)::value - FIRST] = S.a; ro[decltype(L)::value - FIRST] = r;
    });
    const V3 p = r + mul(E, tip);
    ep = pd - p;
    // Rd E^T and its quaternion
    const V3 d0 = mk(Rd.m00, Rd.m01, Rd.m02), d1 = mk(Rd.m10, Rd.m11, Rd.m12), d2 = mk(Rd.m20, Rd.m21, Rd.m22);
    const V3 e0 = mk(E.m00, E.m01, E.m02), e1 = mk(E.m10, E.m11, E.m12), e2 = mk(E.m20, E.m21, E.m22);
    const M3 Re = {dot(d0, e0), dot(d0, e1), dot(d0, e2), dot(d1, e0), dot(d1, e1), dot(d1, e2), dot(d2, e0), dot(d2, e1), dot(d2, e2)};
    float qe[4];
    mat_to_quat(Re, qe);
    const float sg = qe[3] < 0.f ? -2.f : 2.f;
    er = mk(sg * qe[0], sg * qe[1], sg * qe[2]);
    if (it >= K.iters) break;
    V3 Jl[LEN];
#pragma unroll
    for (int i = 0; i < LEN; ++i) Jl[i] = cross(a[i], p - ro[i]);
    // the lower triangle of J^T W J + lambda^2 I, factored in place as L L^T; b = J^T W e
    float A[LEN][LEN], inv[LEN], x[LEN];
#pragma unroll
    for (int i = 0; i < LEN; ++i) {
#pragma unroll
      for (int j = 0; j <= i; ++j) A[i][j] = fmaf(wp, dot(Jl[i], Jl[j]), wr * dot(a[i], a[j]));
      A[i][i] += K.lam2;
      x[i] = fmaf(wp, dot(Jl[i], ep), wr * dot(a[i], er));
    }
    chol_factor<LEN>(A, inv);
    chol_solve<LEN>(A, inv, x);
    float big = 0.f;
#pragma unroll
    for (int i = 0; i < LEN; ++i) big = fmaxf(big, fabsf(x[i]));
    const float sc = (K.max_step > 0.f && big > K.max_step) ? K.max_step / big : 1.f;
#pragma unroll
    for (int i = 0; i < LEN; ++i) {
      const float dq = x[i] * sc;
      q[i] = ik_clamp(q[i] + dq, lo[i], hi[i]) + (dq - dq);   // (dq - dq: 0 for a finite step, NaN for an infinite one, which the limits would hide)
    }
  }
#pragma unroll
  for (int i = 0; i < LEN; ++i) Q[D0 + i] = q[i];
  R[0] = ep.x; R[1] = ep.y; R[2] = ep.z; R[3] = er.x; R[4] = er.y; R[5] = er.z;
}
template <bool CL>
__global__ void __launch_bounds__(IK_THREADS) limb_ik_kernel(DynArgs D, const float* __restrict__ lower, const float* __restrict__ upper,
                                                             const float* __restrict__ targets, BezIkParams P, float* __restrict__ q_out,
                                                             float* __restrict__ err_out) {
  __shared__ float trows[IK_TILE * IK_TSTRIDE];
  __shared__ float qrows[IK_TILE * IK_QSTRIDE];
  __shared__ float erows[IK_TILE * IK_ESTRIDE];
  const int n = D.n, e0 = blockIdx.x * IK_TILE, ne = min(IK_TILE, n - e0);
  tile_load<IK_TW, IK_TSTRIDE, IK_THREADS>(trows, targets + (size_t)e0 * IK_TW, ne);
  __syncthreads();
  const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
  if (lane < ne) {
    const int e = e0 + lane;
    IkCtx K = {D, lower, upper, e, quirk_rz<CL>(D.flags), P.space == BEZ_IK_SPACE_ENV, {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f},
               mk(0.f, 0.f, 0.f), P.damping * P.damping, P.max_step, P.iters};
    if (K.env) {   // (ROOT targets: the root pose is not read)
      K.E0 = root_rotation(D, e);
      K.root_pos = state3_at(D, F_ROOT_POS, e);
    }
    static_for<BEZ_IK_CHAINS>([&](auto Ci) {
      constexpr int c = decltype(Ci)::value;
      if (wave == c) {
        asm volatile("" : "+v"(K.e));   // (opaque per chain, as in inverse_dynamics_kernel)
        ik_chain<CL, c>(K, P, trows + lane * IK_TSTRIDE + 7 * c, qrows + lane * IK_QSTRIDE, erows + lane * IK_ESTRIDE + 6 * c);
      }
    });
  }
  __syncthreads();
  if (q_out) tile_store<BEZ_ND, IK_QSTRIDE, IK_THREADS>(qrows, q_out + (size_t)e0 * BEZ_ND, ne);
  if (err_out) tile_store<IK_EW, IK_ESTRIDE, IK_THREADS>(erows, err_out + (size_t)e0 * IK_EW, ne);
}

// ---- bez_sim_forward_dynamics (definition: include/bez_sim.h "Forward dynamics"): udot = M^-1 (f - h), solved on the tree's structure.
// The tree is a torso and five chains whose joints are disjoint, so the blocks of M between different chains are exact zeros and M is
// a block arrow: [M00 B^T; B diag(M_cc)] with M00 the 6 x 6 base block, M_cc the k x k joint block of chain c (k = 2 or 6) and B_c its
// k x 6 coupling to the base, the rows F_l = I^c_l S_l of its links.  Eliminating the chains leaves the Schur complement on the base:
//     y_c = M_cc^-1 r_c,  Z_c = M_cc^-1 B_c,  S = M00 - sum_c B_c^T Z_c,  g = r_0 - sum_c B_c^T y_c,  x_0 = S^-1 g,  x_c = y_c - Z_c x_0
// with r = f - h.  Nothing larger than 6 x 6 is factored, and no 24 x 24 matrix is held anywhere.
// A workgroup is four waves and takes FD_TILE consecutive envs; a unit is FD_TILE consecutive lanes, one per env of the tile.  All
// lanes bring the tile's force rows into LDS (tile_load; zeros for a null pointer, in the one loop that also zeroes the bias rows --
// tile_load_or_zero would pass over the tile a second time for them).  Then two waves work at once: unit 0 (wave 0) walks
// the tree for h (fd_bias) with the bias terms asked for and leaves it in the env's second row; unit 4 (wave 1) runs phase 1 of
// refresh_dynamics_kernel (dyn_joint_words, dyn_mass_words) and leaves the base block and the F_l in the env's MS_* words.  Then every
// chain has a unit of its own, as in limb_ik_kernel -- the legs and the right arm a wave each, the head and the left arm (2 x 2
// problems) the first two units of wave 0, which runs them one after the other: the unit walks its chain for M_cc (fd_chain_block), reads B_c through
// the slot table of the mass matrix, factors M_cc (chol_factor) and keeps y_c and the six columns of Z_c in registers; the 21 distinct values of
// B_c^T Z_c and the 6 of B_c^T y_c go to the chain's words of the env.  Unit 0 then forms S and g, the chains' parts taken off in the
// fixed order c = 0 .. 4, factors S, and writes x_0 over the force row's first six words; the chains' units finish with x_c = y_c -
// Z_c x_0 over their own words of that row, and all lanes store the tile's rows (tile_store).
// (Four waves, not one per chain: a fifth wave shares a SIMD with another, which caps every wave at 256 registers, and the 19 link
// frames that phase 1 keeps live need 10 more -- the compiler then spills 14 registers to 60 bytes of scratch per lane.)
// BEZ_FD_FIXED_BASE: x_0 = +0.0f, x_c = y_c -- no Z_c, no Schur complement; a chain's result then depends on its own rows alone.
// An env's values pass through that env's lanes and LDS words only: its bits depend neither on N nor on its place in the tile, and a
// non-finite input stays in its env.  Every result is canonicalised (x + 0.0f).
constexpr int FD_TILE = 16, FD_THREADS = 256, FD_RSTRIDE = DYN_NG + 1;   // odd row strides: the lanes' own rows start in distinct LDS banks
constexpr int FD_CW = 21 + 6, FD_CSTRIDE = (FD_CW * BEZ_IK_CHAINS) | 1;                 // a chain's words: tri(B^T Z), B^T y
constexpr int fd_unit(int c) { return c < 2 ? c : 4 * (c - 1); }                        // the unit that takes chain c
static_assert(FD_TILE == DYN_TILE && 64 % FD_TILE == 0 && (fd_unit(BEZ_IK_CHAINS - 1) + 1) * FD_TILE <= FD_THREADS, "units of one lane per env; the tile of refresh_dynamics_kernel");
constexpr int fd_tri(int a, int b) { return a * (a + 1) / 2 + b; }   // (a, b), a >= b, of a lower triangle stored row by row
// M[I][J] of the env whose MS_* words start at Ms
template <int I, int J>
BEZ_DEV float mass_at(const float* Ms) {
  constexpr int slot = MASS_SLOT_TABLE.s[I * DYN_NG + J];
  return Ms[slot];
}
// Link L's mass, its centre of mass c (E, r: the link's frame) and its inertia about c in the axes of E's columns: link_inertia's
// inputs, not moved to the origin of r
template <int L, bool CL>
BEZ_DEV void link_com_inertia(float ms, const M3& E, V3 r, float& m, V3& c, Sym3& Iw) {
  m = (float)link_mass<CL>(L) * ms;
  c = r + mul(E, mk((float)link_com<CL>(L, 0), (float)link_com<CL>(L, 1), (float)link_com<CL>(L, 2)));
  Sym3 Il;
  Il.xx = (float)link_inertia_c<CL>(L, 0) * ms; Il.yy = (float)link_inertia_c<CL>(L, 1) * ms; Il.zz = (float)link_inertia_c<CL>(L, 2) * ms;
  Il.xy = (float)link_inertia_c<CL>(L, 3) * ms; Il.xz = (float)link_inertia_c<CL>(L, 4) * ms; Il.yz = (float)link_inertia_c<CL>(L, 5) * ms;
  constexpr bool DIAG = link_inertia_c<CL>(L, 3) == 0. && link_inertia_c<CL>(L, 4) == 0. && link_inertia_c<CL>(L, 5) == 0.;
  Iw = DIAG ? rotate_inertia_diag(E, Il.xx, Il.yy, Il.zz) : rotate_inertia(E, Il);
}
// The lower triangle of M_cc, chain C's joint block of M, with every lever arm taken from the joint's own origin:
//     M_ij = sum over the links l at or below joint i of  m_l (a_i x (c_l - r_i)) . (a_j x (c_l - r_j)) + a_j . I_l a_i  (+ armature, i = j)
// in the root's axes (the block does not depend on the root's pose).  The MS_PAIR words of refresh_dynamics_kernel hold the same
// numbers as a_j . (F.a - r_j x F.l) with F = I^c_i S_i about the ROOT origin: a moment of the size m |r|^2 taken back to the joint, which
// leaves 2.3e-6 of sqrt(M_ii M_jj) in them.  The solve multiplies that by M_cc^-1: measured on MI355X, the joint rows
// of udot = M^-1 f then miss the fp64 reference by 1.1e-3 rad/s^2 of 500, of which the fp32 elimination itself accounts for 2e-4.
template <bool CL, int C>
BEZ_DEV void fd_chain_block(const DynArgs& D, int e, float (&A)[chain_len(C)][chain_len(C)]) {
  constexpr int FIRST = chain_first(C), LEN = chain_len(C);
  M3 E = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
  V3 r = mk(0.f, 0.f, 0.f), a[LEN], ro[LEN];
  still_chain_walk<FIRST, LEN>(E, r, quirk_rz<CL>(D.flags), [&](auto Lk) { return state_at(D, F_Q + decltype(Lk)::value - 1, e); }, [&](auto Lk, const SV& S) {
    constexpr int l = decltype(Lk)::value - FIRST;
    a[l] = S.a; ro[l] = r;
    float m; V3 c; Sym3 Iw;
    link_com_inertia<FIRST + l, CL>(mass_scale_of(D, e, FIRST + l), E, r, m, c, Iw);
    V3 u[l + 1], w[l + 1];
#pragma unroll
    for (int i = 0; i <= l; ++i) { u[i] = cross(a[i], c - ro[i]); w[i] = mul(Iw, a[i]); }
#pragma unroll
    for (int i = 0; i <= l; ++i) {
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        const float v = fmaf(m, dot(u[i], u[j]), dot(a[j], w[i]));
        A[i][j] = (i == l) ? (i == j ? v + D.armature : v) : A[i][j] + v;   // (row l starts with link l)
      }
    }
  });
}
// Chain C of one env.  Ms: the env's MS_* words; F, H: its force and bias rows; W: the chain's FD_CW words; y, Z: what the chain keeps
// for fd_chain_finish (the first LEN rows are used)
template <bool CL, int C>
BEZ_DEV void fd_chain_reduce(const DynArgs& D, int e, const float* Ms, const float* F, const float* H, bool floating, float* W, float (&y)[6],
                             float (&Z)[6][6]) {
  constexpr int LEN = chain_len(C), R0 = 5 + chain_first(C);   // the chain's first row of M
  static_assert(LEN <= 6, "a chain's factor is at most 6 x 6");
  float A[LEN][LEN], inv[LEN], x[LEN];
  fd_chain_block<CL, C>(D, e, A);
#pragma unroll
  for (int i = 0; i < LEN; ++i) x[i] = F[R0 + i] - H[R0 + i];
  chol_factor<LEN>(A, inv);
  chol_solve<LEN>(A, inv, x);
#pragma unroll
  for (int i = 0; i < LEN; ++i) y[i] = x[i];
  if (!floating) return;
  float B[LEN][6];
  static_for<LEN>([&](auto I) {
    constexpr int i = decltype(I)::value;
    static_for<6>([&](auto K) { B[i][decltype(K)::value] = mass_at<R0 + i, decltype(K)::value>(Ms); });
  });
#pragma unroll
  for (int k = 0; k < 6; ++k) {
#pragma unroll
    for (int i = 0; i < LEN; ++i) x[i] = B[i][k];
    chol_solve<LEN>(A, inv, x);
#pragma unroll
    for (int i = 0; i < LEN; ++i) Z[i][k] = x[i];
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) {
#pragma unroll
    for (int b = 0; b <= a; ++b) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < LEN; ++i) s = fmaf(B[i][a], Z[i][b], s);
      W[fd_tri(a, b)] = s;
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < LEN; ++i) s = fmaf(B[i][a], y[i], s);
    W[21 + a] = s;
  }
}
// x_c = y_c - Z_c x_0 (fixed base: y_c) into the chain's words of the env's row X, whose first six words hold x_0
template <int C>
BEZ_DEV void fd_chain_finish(bool floating, float* X, const float (&y)[6], const float (&Z)[6][6]) {
  constexpr int LEN = chain_len(C), R0 = 5 + chain_first(C);
  float x0[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) x0[k] = floating ? X[k] : 0.f;
#pragma unroll
  for (int i = 0; i < LEN; ++i) {
    float x = y[i];
    if (floating) {
#pragma unroll
      for (int k = 0; k < 6; ++k) x = fmaf(-Z[i][k], x0[k], x);
    }
    X[R0 + i] = x + 0.f;
  }
}
// The base of one env: S = M00 - sum_c B_c^T Z_c and g = r_0 - sum_c B_c^T y_c from the chains' words W, x_0 = S^-1 g over X[0:6]
BEZ_DEV void fd_base_solve(const float* Ms, const float* H, const float* W, float* X) {
  float S[6][6], inv[6], g[6];
  static_for<6>([&](auto I) {
    constexpr int i = decltype(I)::value;
    static_for<i + 1>([&](auto J) {
      constexpr int j = decltype(J)::value;
      float s = mass_at<i, j>(Ms);
#pragma unroll
      for (int c = 0; c < BEZ_IK_CHAINS; ++c) s -= W[FD_CW * c + fd_tri(i, j)];
      S[i][j] = s;
    });
    float s = X[i] - H[i];
#pragma unroll
    for (int c = 0; c < BEZ_IK_CHAINS; ++c) s -= W[FD_CW * c + 21 + i];
    g[i] = s;
  });
  chol_factor<6>(S, inv);
  chol_solve<6>(S, inv, g);
#pragma unroll
  for (int i = 0; i < 6; ++i) X[i] = g[i] + 0.f;
}
// h(q, u) of one env, the terms in `bias`, into its row H: the walk of inverse_dynamics_kernel with udot = 0 and every link's wrench taken
// about the LINK's own origin (world axes), where the joint torque is a . n.  id_links takes all moments about the root origin: a
// distal joint's torque is then what is left of moments of 0.3 m x 75 N (the test states turn joints at 20 rad/s), and that rounding,
// harmless in a force, is multiplied by M_cc^-1 here -- measured on MI355X with h from id_links, the joint rows of udot missed their
// bar by 1.15 on states with a mass-scale row.  On the way back a link hands its subtree's wrench to its parent's origin, a lever arm
// of one link.  The velocity product and gravity are link_inertia's own bias force pA = v x* I v - I [0; g].
template <int L, int END, bool CL>
BEZ_DEV SV fd_bias_links(const IdCtx& C, M3 E, V3 r, SV V, SV aV, float* H) {
  const V3 r_parent = r;
  const float q = state_at(C.D, F_Q + L - 1, C.e), qd = C.vel ? state_at(C.D, F_QD + L - 1, C.e) : 0.f;
  SV S, cb;
  link_kinematics<L>(q, qd, E, r, V, S, cb, C.quirk_z);
  aV = aV + cb;
  // the link's velocity and acceleration about its own origin (V, aV: about the root origin)
  const SV Vl = mksv(V.a, point_of(V, r)), al = mksv(aV.a, point_of(aV, r));
  LinkInertia LI; SV F;
  link_inertia<L, CL>(mass_scale_of(C.D, C.e, L), C.g, E, mk(0.f, 0.f, 0.f), Vl, LI, F);
  F = F + inertia_times(LI, al);
  if constexpr (L + 1 < END) F = F + fd_bias_links<L + 1, END, CL>(C, E, r, V, aV, H);
  H[5 + L] = dot(S.a, F.a);
  return mksv(F.a + cross(r - r_parent, F.l), F.l);
}
template <bool CL>
BEZ_DEV void fd_bias(const DynArgs& D, int e, uint32_t bias, float* H) {
  const bool vel = (bias & BEZ_ID_VELOCITY) != 0;
  const M3 E0 = root_rotation(D, e);
  const SV V0 = vel ? mksv(state3_at(D, F_ROOT_ANG, e), state3_at(D, F_ROOT_LIN, e)) : svzero();
  V3 g = mk(0.f, 0.f, 0.f);
  if (bias & BEZ_ID_GRAVITY) g = gravity_of(D, e);
  const SV aV0 = mksv(mk(0.f, 0.f, 0.f), -cross(V0.a, V0.l));   // (inverse_dynamics_kernel: the torso's acceleration about a fixed point)
  LinkInertia I0; SV F0;
  link_inertia<0, CL>(mass_scale_of(D, e, 0), g, E0, mk(0.f, 0.f, 0.f), V0, I0, F0);
  F0 = F0 + inertia_times(I0, aV0);
  IdCtx C = {D, e, vel, quirk_rz<CL>(D.flags), g};
  for_each_chain<true>([&](auto first, auto len) {
    constexpr int FIRST = decltype(first)::value, LEN = decltype(len)::value;
    asm volatile("" : "+v"(C.e), "+v"(F0.l.x));   // (opaque per chain, as in inverse_dynamics_kernel)
    F0 = F0 + fd_bias_links<FIRST, FIRST + LEN, CL>(C, E0, mk(0.f, 0.f, 0.f), V0, aV0, H);
  });
  H[0] = F0.l.x; H[1] = F0.l.y; H[2] = F0.l.z; H[3] = F0.a.x; H[4] = F0.a.y; H[5] = F0.a.z;
}
template <bool CL>
__global__ void __launch_bounds__(FD_THREADS) forward_dynamics_kernel(DynArgs D, const float* force, float* out, uint32_t bias, int fixed) {
  __shared__ float lds[FD_TILE * DYN_STRIDE];
  __shared__ float frows[FD_TILE * FD_RSTRIDE];   // f, then udot
  __shared__ float hrows[FD_TILE * FD_RSTRIDE];   // h
  __shared__ float crows[FD_TILE * FD_CSTRIDE];
  const int n = D.n, e0 = blockIdx.x * FD_TILE, ne = min(FD_TILE, n - e0);
  if (force) tile_load<DYN_NG, FD_RSTRIDE, FD_THREADS>(frows, force + (size_t)e0 * DYN_NG, ne);
  for (int i = threadIdx.x; i < ne * DYN_NG; i += FD_THREADS) {
    if (!force) frows[tile_word<DYN_NG, FD_RSTRIDE>(i)] = 0.f;
    hrows[tile_word<DYN_NG, FD_RSTRIDE>(i)] = 0.f;
  }
  __syncthreads();
  const int el = threadIdx.x % FD_TILE, unit = threadIdx.x / FD_TILE;
  const bool mine = el < ne, floating = !fixed;
  const int e = e0 + el;
  float* L = lds + el * DYN_STRIDE;
  float* X = frows + el * FD_RSTRIDE;
  const float* H = hrows + el * FD_RSTRIDE;
  float* W = crows + el * FD_CSTRIDE;
  if (mine && unit == 0 && bias) fd_bias<CL>(D, e, bias, hrows + el * FD_RSTRIDE);
  if (mine && unit == 4) {
    EnvState S;
    load_state(D.st, n, e, S);
    M3 E[BEZ_NL]; V3 r[BEZ_NL]; SV V[BEZ_NL];
    link_frames<CL, false>(S, D.flags, E, r, V);
    dyn_joint_words(L, E, r);
    dyn_mass_words<CL, false>(D, e, L, E, r);
  }
  __syncthreads();
  float y[6], Z[6][6];
  static_for<BEZ_IK_CHAINS>([&](auto Ci) {
    constexpr int c = decltype(Ci)::value;
    if (mine && unit == fd_unit(c)) fd_chain_reduce<CL, c>(D, e, L + DYN_MS, X, H, floating, W + FD_CW * c, y, Z);
  });
  __syncthreads();
  if (mine && unit == 0) {
    if (floating) fd_base_solve(L + DYN_MS, H, W, X);
    else {
#pragma unroll
      for (int i = 0; i < 6; ++i) X[i] = 0.f;
    }
  }
  __syncthreads();
  static_for<BEZ_IK_CHAINS>([&](auto Ci) {
    constexpr int c = decltype(Ci)::value;
    if (mine && unit == fd_unit(c)) fd_chain_finish<c>(floating, X, y, Z);
  });
  __syncthreads();
  tile_store<DYN_NG, FD_RSTRIDE, FD_THREADS>(frows, out + (size_t)e0 * DYN_NG, ne);
}

// ---- bez_sim_operational_space (definition: include/bez_sim.h "Operational space"): the 30 columns J_E^T of the five controlled frames
// solved on forward_dynamics_kernel's one factorisation of the block arrow.  Column block c of J_E^T is non-zero on the base rows (X_c^T,
// X_c = [I -skew(x); 0 I]) and on chain c's rows (J_cc^T) alone, so with y_c = M_cc^-1 J_cc^T, Z_c = M_cc^-1 B_c and S = L L^T the Schur
// complement:
//     P_c = X_c - J_cc Z_c  (= G_c^T, G_c = X_c^T - B_c^T y_c),   Q_c = L^-1 P_c^T,   x_0^(c) = S^-1 P_c^T = L^-T Q_c,
//     chain a's rows of M^-1 J_c^T:  delta_ac y_c - Z_a x_0^(c),
//     W_ab = X_a x_0^(b) + J_aa x_a^(b) = Q_a^T Q_b + delta_ab J_aa y_a,     Lambda_c = W_cc^-1.
// W in the Q form is a Gram matrix plus the chain's own block: it is symmetric term by term, and what is left of S's rounding enters
// both factors alike.  J_cc's levers are a_j x (p - r_j) from the joint's own origin in the root's axes (ik_chain's), turned to world
// axes by the root's rotation as whole vectors.
// The tile, the units and phase 1 are forward_dynamics_kernel's.  Unit 4 leaves M00 and the F_l in the env's MS_* words; then every chain's
// unit walks its chain twice (fd_chain_block for M_cc, still_chain_walk for J_cc and the controlled point), factors M_cc and leaves Z_c,
// y_c, J_cc, x, tri(B_c^T Z_c) and tri(J_cc y_c) in the env's OS_* words, keeping P_c in registers; unit 0 factors S and publishes the
// tri-packed factor and its reciprocals; the chains' units solve their own six columns for Q_c and x_0^(c), finish their own rows
// y_c - Z_c x_0^(c) and W_cc in place, and invert W_cc by a 6 x 6 Cholesky.  Last, all lanes form the outputs element by element from the
// env's words in the order of the tile's contiguous output ranges and store them as float4 (refresh_dynamics_kernel's phase 2; a range
// that is not 16-byte aligned: the scalar path to the same bits): a tile's outputs are 161 KB, and none of them is staged.  Both
// triangles of w take one value: every element is formed from the sorted pair of its indices.
// The words of phase 1 (and the chains' B^T Z) are dead once S is factored: Q, x_0 and Lambda are laid over them, which keeps the
// tile under 64 KB.  BEZ_FD_FIXED_BASE: no phase 1, no Z, no S; x_0 = 0, W_cc = J_cc y_c, and every structural zero is a literal.
// An env's values pass through that env's lanes and LDS words only.
constexpr int OS_TILE = FD_TILE, OS_THREADS = FD_THREADS, OS_NF = 6 * BEZ_IK_CHAINS;
constexpr int OS_BZ = DYN_STRIDE;                                                                       // live until S is factored
constexpr int OS_Q = 0, OS_X0 = OS_Q + 36 * BEZ_IK_CHAINS, OS_LAM = OS_X0 + 36 * BEZ_IK_CHAINS;         // laid over them afterwards
constexpr int OS_SF = (OS_BZ > OS_LAM ? OS_BZ : OS_LAM) + 21 * BEZ_IK_CHAINS;                           // tri(L), 1 / diag(L); then tri(S)
constexpr int OS_S0 = OS_SF + 27, OS_Z = OS_S0 + 21, OS_XC = OS_Z + 6 * BEZ_ND, OS_JL = OS_XC + 6 * BEZ_ND, OS_JA = OS_JL + 3 * BEZ_ND, OS_XP = OS_JA + 3 * BEZ_ND;
constexpr int OS_WD = OS_XP + 3 * BEZ_IK_CHAINS, OS_STRIDE = (OS_WD + 21 * BEZ_IK_CHAINS) | 1;          // odd, as DYN_STRIDE
static_assert(OS_TILE * OS_STRIDE * sizeof(float) <= 65536, "the tile's words fit the static LDS limit");
constexpr int os_chain_of_dof(int d) { int c = 0; for (int k = 1; k < BEZ_IK_CHAINS; ++k) c += d >= chain_first(k) - 1; return c; }
// the two halves of chol_solve
template <int K>
BEZ_DEV void chol_forward(const float (&A)[K][K], const float (&inv)[K], float (&x)[K]) {
#pragma unroll
  for (int i = 0; i < K; ++i) {
#pragma unroll
    for (int k = 0; k < i; ++k) x[i] = fmaf(-A[i][k], x[k], x[i]);
    x[i] *= inv[i];
  }
}
template <int K>
BEZ_DEV void chol_backward(const float (&A)[K][K], const float (&inv)[K], float (&x)[K]) {
#pragma unroll
  for (int i = K - 1; i >= 0; --i) {
#pragma unroll
    for (int k = i + 1; k < K; ++k) x[i] = fmaf(-A[k][i], x[k], x[i]);
    x[i] *= inv[i];
  }
}
// Chain C of one env up to the Schur complement.  O: the env's words; P: P_C, kept for os_chain_finish (floating base alone)
template <bool CL, int C>
BEZ_DEV void os_chain_reduce(const DynArgs& D, int e, const BezOpSpaceParams& Pm, bool floating, float* O, float (&P)[6][6]) {
  constexpr int FIRST = chain_first(C), LEN = chain_len(C), D0 = FIRST - 1, R0 = 5 + FIRST;
  float A[LEN][LEN], inv[LEN], x[LEN];
  fd_chain_block<CL, C>(D, e, A);
  float A0[LEN][LEN];   // M_cc itself, for the residuals of Z_c
#pragma unroll
  for (int i = 0; i < LEN; ++i) {
#pragma unroll
    for (int j = 0; j <= i; ++j) A0[i][j] = A0[j][i] = A[i][j];
  }
  chol_factor<LEN>(A, inv);
  // J_cc = [E0 (a_j x (p - r_j)); E0 a_j] and the controlled point x = E0 p
  float J[6][LEN];
  V3 xw;
  {
    M3 E = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    V3 r = mk(0.f, 0.f, 0.f), a[LEN], ro[LEN];
    still_chain_walk<FIRST, LEN>(E, r, quirk_rz<CL>(D.flags), [&](auto Lk) { return state_at(D, F_Q + decltype(Lk)::value - 1, e); }, [&](auto Lk, const SV& S) {
      a[decltype(Lk)::value - FIRST] = S.a; ro[decltype(Lk)::value - FIRST] = r;
    });
    const BodyFrame bf = body_frame<CL>(link_body<CL>(FIRST + LEN - 1));
    const V3 p = r + mul(E, bf.off + mk(Pm.offset[C][0], Pm.offset[C][1], Pm.offset[C][2]));
    const M3 E0 = root_rotation(D, e);
    xw = mul(E0, p);
    dyn_put3(O, OS_XP + 3 * C, xw);
#pragma unroll
    for (int i = 0; i < LEN; ++i) {
      const V3 jl = mul(E0, cross(a[i], p - ro[i])), ja = mul(E0, a[i]);
      J[0][i] = jl.x; J[1][i] = jl.y; J[2][i] = jl.z; J[3][i] = ja.x; J[4][i] = ja.y; J[5][i] = ja.z;
      dyn_put3(O, OS_JL + 3 * (D0 + i), jl);
      dyn_put3(O, OS_JA + 3 * (D0 + i), ja);
    }
  }
  if (floating) {
    const float* Ms = O + DYN_MS;
    float B[LEN][6], Z[LEN][6];
    static_for<LEN>([&](auto I) {
      constexpr int i = decltype(I)::value;
      static_for<6>([&](auto K) { B[i][decltype(K)::value] = mass_at<R0 + i, decltype(K)::value>(Ms); });
    });
#pragma unroll
    for (int k = 0; k < 6; ++k) {
#pragma unroll
      for (int i = 0; i < LEN; ++i) x[i] = B[i][k];
      chol_solve<LEN>(A, inv, x);
      // one step of refinement on the column, the residual against M_cc in fp64: P_c = X_c - J_cc Z_c is what is left of X_c
      float d[LEN];
#pragma unroll
      for (int i = 0; i < LEN; ++i) {
        double r = B[i][k];
#pragma unroll
        for (int m = 0; m < LEN; ++m) r = fma(-(double)A0[i][m], (double)x[m], r);
        d[i] = (float)r;
      }
      chol_solve<LEN>(A, inv, d);
#pragma unroll
      for (int i = 0; i < LEN; ++i) { x[i] += d[i]; Z[i][k] = x[i]; O[OS_Z + 6 * (D0 + i) + k] = x[i]; }
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
      for (int b = 0; b <= a; ++b) {
        double s = 0.0;   // (fp64: the products of two floats are exact, and S is what is left of M00 after these are taken off)
#pragma unroll
        for (int i = 0; i < LEN; ++i) s = fma((double)B[i][a], (double)Z[i][b], s);
        O[OS_BZ + 21 * C + fd_tri(a, b)] = (float)s;
      }
    }
    const float X[3][3] = {{0.f, xw.z, -xw.y}, {-xw.z, 0.f, xw.x}, {xw.y, -xw.x, 0.f}};   // -skew(x)
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        float s = (i < 3 && k >= 3) ? X[i % 3][k % 3] : (i == k ? 1.f : 0.f);
#pragma unroll
        for (int r = 0; r < LEN; ++r) s = fmaf(-J[i][r], Z[r][k], s);
        P[i][k] = s;
      }
    }
  }
  // y_c column by column, and the lower triangle of J_cc y_c
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int r = 0; r < LEN; ++r) x[r] = J[i][r];
    chol_solve<LEN>(A, inv, x);
#pragma unroll
    for (int r = 0; r < LEN; ++r) O[OS_XC + 6 * (D0 + r) + i] = x[r];
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      float s = 0.f;
#pragma unroll
      for (int r = 0; r < LEN; ++r) s = fmaf(J[j][r], x[r], s);
      O[OS_WD + 21 * C + fd_tri(i, j)] = s;
    }
  }
}
// S = M00 - sum_c B_c^T Z_c of one env (fd_base_solve's sum), factored; the factor's lower triangle and reciprocals go to OS_SF
BEZ_DEV void os_base_factor(float* O) {
  const float* Ms = O + DYN_MS;
  float S[6][6], inv[6];
  static_for<6>([&](auto I) {
    constexpr int i = decltype(I)::value;
    static_for<i + 1>([&](auto Jc) {
      constexpr int j = decltype(Jc)::value;
      double s = mass_at<i, j>(Ms);
#pragma unroll
      for (int c = 0; c < BEZ_IK_CHAINS; ++c) s -= (double)O[OS_BZ + 21 * c + fd_tri(i, j)];
      S[i][j] = (float)s;
      O[OS_S0 + fd_tri(i, j)] = S[i][j];
    });
  });
  chol_factor<6>(S, inv);
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = 0; j <= i; ++j) O[OS_SF + fd_tri(i, j)] = S[i][j];
    O[OS_SF + 21 + i] = inv[i];
  }
}
// Chain C of one env behind the Schur complement: Q_C and x_0^(C), the chain's own rows y_C - Z_C x_0^(C) over y_C, W_CC over J_CC y_C,
// Lambda_C where it is asked for
template <int C>
BEZ_DEV void os_chain_finish(bool floating, bool want_lambda, float* O, const float (&P)[6][6]) {
  constexpr int LEN = chain_len(C), D0 = chain_first(C) - 1;
  float Wc[6][6];
  double Wd[6][6];   // W_CC before its rounding to fp32, for Lambda's residual
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = 0; j <= i; ++j) { Wc[i][j] = O[OS_WD + 21 * C + fd_tri(i, j)]; Wd[i][j] = Wd[j][i] = Wc[i][j]; }
  }
  if (floating) {
    float S[6][6], S0[6][6], inv[6], Q[6][6], X0[6][6], x[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
      for (int j = 0; j <= i; ++j) { S[i][j] = O[OS_SF + fd_tri(i, j)]; S0[i][j] = S0[j][i] = O[OS_S0 + fd_tri(i, j)]; }
      inv[i] = O[OS_SF + 21 + i];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
      for (int k = 0; k < 6; ++k) x[k] = P[i][k];
      chol_forward<6>(S, inv, x);
#pragma unroll
      for (int k = 0; k < 6; ++k) { Q[k][i] = x[k]; O[OS_Q + 36 * C + 6 * k + i] = x[k]; }
      chol_backward<6>(S, inv, x);
      // one step of refinement on the column: the residual against S in fp64
      float d[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        double r = P[i][k];
#pragma unroll
        for (int m = 0; m < 6; ++m) r = fma(-(double)S0[k][m], (double)x[m], r);
        d[k] = (float)r;
      }
      chol_solve<6>(S, inv, d);
#pragma unroll
      for (int k = 0; k < 6; ++k) { x[k] += d[k]; X0[k][i] = x[k]; O[OS_X0 + 36 * C + 6 * k + i] = x[k]; }
    }
#pragma unroll
    for (int r = 0; r < LEN; ++r) {
      float z[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) z[k] = O[OS_Z + 6 * (D0 + r) + k];
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        float s = O[OS_XC + 6 * (D0 + r) + i];
#pragma unroll
        for (int k = 0; k < 6; ++k) s = fmaf(-z[k], X0[k][i], s);
        O[OS_XC + 6 * (D0 + r) + i] = s;
      }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        double s = Wc[i][j];
#pragma unroll
        for (int k = 0; k < 6; ++k) s = fma((double)Q[k][i], (double)Q[k][j], s);
        Wd[i][j] = Wd[j][i] = s;
        Wc[i][j] = (float)s;
        O[OS_WD + 21 * C + fd_tri(i, j)] = Wc[i][j];
      }
    }
  }
  if (want_lambda) {
    // Lambda = W_cc^-1 column by column from the factor of the rounded block, then one Newton step Lambda += Lambda (I - W_cc Lambda)
    // whose residual is formed in fp64 against the UNROUNDED W_cc (Wd): cond(W_cc) reaches 6e3, and what Lambda loses is the rounding of
    // W_cc's entries to fp32, not the inversion -- measured on MI355X 1.43 of the known-answer bar with the residual against the
    // rounded block, 0.86 against Wd
    float Lm[6][6], inv[6], x[6];
    chol_factor<6>(Wc, inv);
#pragma unroll
    for (int j = 0; j < 6; ++j) {
#pragma unroll
      for (int k = 0; k < 6; ++k) x[k] = k == j ? 1.f : 0.f;
      chol_solve<6>(Wc, inv, x);
#pragma unroll
      for (int i = j; i < 6; ++i) Lm[i][j] = Lm[j][i] = x[i];
    }
    float R[6][6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        double r = k == j ? 1.0 : 0.0;
#pragma unroll
        for (int m = 0; m < 6; ++m) r = fma(-Wd[k][m], (double)Lm[m][j], r);
        R[k][j] = (float)r;
      }
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
#pragma unroll
      for (int i = j; i < 6; ++i) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 6; ++k) s = fmaf(Lm[i][k], R[k][j], s);
        O[OS_LAM + 21 * C + fd_tri(i, j)] = Lm[i][j] + s;
      }
    }
  }
}
// Element i of an env's output from its words O: jac (5, 6, 24), jminv (5, 6, 24), w (30, 30), lambda (5, 6, 6)
BEZ_DEV float os_jac_at(const float* O, int i) {
  const int col = i % DYN_NG, row = (i / DYN_NG) % 6, c = i / (6 * DYN_NG);
  if (col < 6) return jacobian_entry(O, 0u, lds3(O + OS_XP + 3 * c), row, col);
  const int d = col - 6;
  if (os_chain_of_dof(d) != c) return 0.f;
  return row < 3 ? O[OS_JL + 3 * d + row] : O[OS_JA + 3 * d + row - 3];
}
BEZ_DEV float os_jminv_at(const float* O, int i, bool floating) {
  const int col = i % DYN_NG, row = (i / DYN_NG) % 6, b = i / (6 * DYN_NG);
  if (col < 6) return floating ? O[OS_X0 + 36 * b + 6 * col + row] : 0.f;
  const int d = col - 6;
  if (os_chain_of_dof(d) == b) return O[OS_XC + 6 * d + row];
  if (!floating) return 0.f;
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 6; ++k) s = fmaf(-O[OS_Z + 6 * d + k], O[OS_X0 + 36 * b + 6 * k + row], s);
  return s;
}
BEZ_DEV float os_w_at(const float* O, int i, bool floating) {
  const int r = i / OS_NF, c = i % OS_NF, lo = min(r, c), hi = max(r, c), a = lo / 6, ia = lo % 6, b = hi / 6, ib = hi % 6;
  if (a == b) return O[OS_WD + 21 * a + fd_tri(ib, ia)];
  if (!floating) return 0.f;
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 6; ++k) s = fmaf(O[OS_Q + 36 * a + 6 * k + ia], O[OS_Q + 36 * b + 6 * k + ib], s);
  return s;
}
BEZ_DEV float os_lambda_at(const float* O, int i) {
  const int r = (i / 6) % 6, c = i % 6;
  return O[OS_LAM + 21 * (i / 36) + fd_tri(max(r, c), min(r, c))];
}
// the tile's contiguous range of `ne` x PER_ENV elements, each formed by at(the env's words, its index within the env)
template <int PER_ENV, typename At>
BEZ_DEV void os_emit(const float* lds, float* __restrict__ out, int ne, At&& at) {
  static_assert(PER_ENV % 4 == 0, "whole float4s per env");
  auto v = [&](int i) { return at(lds + (i / PER_ENV) * OS_STRIDE, i % PER_ENV); };
  const int count = ne * PER_ENV;
  if ((reinterpret_cast<uintptr_t>(out) & 15u) == 0) {
    float4* o4 = reinterpret_cast<float4*>(out);
    for (int i = threadIdx.x; i < count / 4; i += OS_THREADS) o4[i] = make_float4(v(4 * i), v(4 * i + 1), v(4 * i + 2), v(4 * i + 3));
  } else {
    for (int i = threadIdx.x; i < count; i += OS_THREADS) out[i] = v(i);
  }
}
template <bool CL>
__global__ void __launch_bounds__(OS_THREADS) operational_space_kernel(DynArgs D, BezOpSpaceParams Pm, float* __restrict__ jac, float* __restrict__ jminv,
                                                                       float* __restrict__ w, float* __restrict__ lam) {
  __shared__ float lds[OS_TILE * OS_STRIDE];
  const int n = D.n, e0 = blockIdx.x * OS_TILE, ne = min(OS_TILE, n - e0);
  const int el = threadIdx.x % OS_TILE, unit = threadIdx.x / OS_TILE;
  const bool mine = el < ne, floating = !(Pm.mode & BEZ_FD_FIXED_BASE);
  const int e = e0 + el;
  float* O = lds + el * OS_STRIDE;
  if (mine && unit == 4 && floating) {
    EnvState S;
    load_state(D.st, n, e, S);
    M3 E[BEZ_NL]; V3 r[BEZ_NL]; SV V[BEZ_NL];
    link_frames<CL, false>(S, D.flags, E, r, V);
    dyn_joint_words(O, E, r);
    dyn_mass_words<CL, false>(D, e, O, E, r);
  }
  __syncthreads();
  float P[6][6];
  static_for<BEZ_IK_CHAINS>([&](auto Ci) {
    constexpr int c = decltype(Ci)::value;
    if (mine && unit == fd_unit(c)) os_chain_reduce<CL, c>(D, e, Pm, floating, O, P);
  });
  __syncthreads();
  if (mine && unit == 0 && floating) os_base_factor(O);
  __syncthreads();
  static_for<BEZ_IK_CHAINS>([&](auto Ci) {
    constexpr int c = decltype(Ci)::value;
    if (mine && unit == fd_unit(c)) os_chain_finish<c>(floating, lam != nullptr, O, P);
  });
  __syncthreads();
  if (jac) os_emit<OS_NF * DYN_NG>(lds, jac + (size_t)e0 * (OS_NF * DYN_NG), ne, [](const float* Oe, int i) { return os_jac_at(Oe, i); });
  if (jminv) os_emit<OS_NF * DYN_NG>(lds, jminv + (size_t)e0 * (OS_NF * DYN_NG), ne, [&](const float* Oe, int i) { return os_jminv_at(Oe, i, floating); });
  if (w) os_emit<OS_NF * OS_NF>(lds, w + (size_t)e0 * (OS_NF * OS_NF), ne, [&](const float* Oe, int i) { return os_w_at(Oe, i, floating); });
  if (lam) os_emit<36 * BEZ_IK_CHAINS>(lds, lam + (size_t)e0 * (36 * BEZ_IK_CHAINS), ne, [](const float* Oe, int i) { return os_lambda_at(Oe, i); });
}

// ---- bez_sim_proximity (definition: include/bez_sim.h "Proximity"): the step's three narrow phases -- link_ground_points, test_box_at /
// test_torso_box, segment_closest / self_pair (bez_kernels.h) -- as signed distances that are defined on both sides of contact.
// A workgroup takes PX_TILE consecutive envs.  Phase 1, one lane per env: the chains are walked with still_chain_walk in world
// axes about the root origin (the legs for boxes, capsules and feet; the head and the arms for their guard points alone); the ground rows
// go to the env's output row in LDS, root_pos joining in the last addition, and what the tests need -- the eleven box frames, the twelve
// capsule axes' end points, the ball centre relative to the root origin, root_pos -- to the env's PX_F* words.  Phase 2, all lanes: the
// tile's 16 x (28 + 11) tests, the env fastest, so that every wave runs one kind of test (16 x 28 is a whole number of waves); the
// constants of a test are looked up in PROX_TABLES.  Phase 3, all lanes: the tile's three contiguous ranges are stored with tile_store.
// Rows of odd strides: the lanes of phase 1 write distinct banks.
// The family's form -- one wave, one lane per env that also runs its env's 39 tests, frames and capsules in registers -- computes the
// same bits and was measured on MI355X beside this one (profiles/proximity_tiles.txt).
constexpr int PX_TILE = 16, PX_THREADS = 256;
constexpr int PX_GW = 3 * BEZ_PROX_GROUND_ROWS, PX_BW = BEZ_PROX_WORDS * BEZ_PROX_BOXES, PX_PW = BEZ_PROX_WORDS * BEZ_PROX_PAIRS;
constexpr int PX_GSTRIDE = PX_GW | 1, PX_BSTRIDE = PX_BW | 1, PX_PSTRIDE = PX_PW | 1;
// the PX_F* words of one env: [box frame: E row-major 9, r 3] x 11, [capsule p0 3, p1 3] x 12, ball centre rel. root origin 3, root_pos 3
constexpr int PX_FBOX = 0, PX_FCAP = 12 * BEZ_NBOX, PX_FBALL = PX_FCAP + 6 * BEZ_NCAP, PX_FROOT = PX_FBALL + 3, PX_FSTRIDE = (PX_FROOT + 3) | 1;
static_assert(BEZ_NPT + 1 == BEZ_PROX_GROUND_ROWS && BEZ_NBOX == BEZ_PROX_BOXES && BEZ_NCPAIR == BEZ_PROX_PAIRS, "include/bez_sim.h Proximity");
static_assert(BEZ_TORSO_BOX == BEZ_NBOX - 1, "the torso box is the last entry of the box table");
// box b's centre and half extents (entry BEZ_NBOX: the box asset's torso box), the capsules' radii, the pairs
struct ProxTables { float center[BEZ_NBOX + 1][3], half[BEZ_NBOX + 1][3], cap_r[BEZ_NCAP]; int8_t pair[BEZ_NCPAIR][2]; };
constexpr ProxTables prox_tables() {
  ProxTables T = {};
  for (int k = 0; k < 3; ++k) {
    for (int b = 0; b < BEZ_NBOX; ++b) { T.center[b][k] = (float)BEZ_BOX_CENTER[b][k]; T.half[b][k] = (float)BEZ_BOX_HALF[b][k]; }
    T.center[BEZ_NBOX][k] = (float)BEZ_TORSO_BOX_CENTER_BOX[k]; T.half[BEZ_NBOX][k] = (float)BEZ_TORSO_BOX_HALF_BOX[k];
  }
  for (int c = 0; c < BEZ_NCAP; ++c) T.cap_r[c] = (float)BEZ_CAP_R[c];
  for (int p = 0; p < BEZ_NCPAIR; ++p) { T.pair[p][0] = (int8_t)BEZ_CPAIR[p][0]; T.pair[p][1] = (int8_t)BEZ_CPAIR[p][1]; }
  return T;
}
__device__ const ProxTables PROX_TABLES = prox_tables();
// a row [gap, normal, point, +0.0f]; p is relative to the root origin
BEZ_DEV void prox_put(float* o, float gap, V3 n, V3 p, V3 root_pos) {
  o[BEZ_PROX_GAP] = gap;
  o[BEZ_PROX_NORMAL] = n.x; o[BEZ_PROX_NORMAL + 1] = n.y; o[BEZ_PROX_NORMAL + 2] = n.z;
  o[BEZ_PROX_POINT] = root_pos.x + p.x; o[BEZ_PROX_POINT + 1] = root_pos.y + p.y; o[BEZ_PROX_POINT + 2] = root_pos.z + p.z;
  o[7] = 0.f;
}
// test_box_at as a signed distance: sphere (centre bc rel. O) against the box (centre cl, half extents he) of a link with frame (E, r).
// gap = -depth of test_box_at, kept when positive; n: world normal box -> ball; p: closest point of the box surface rel. O.
// (sqrtf and the division are the correctly rounded ones: nothing here feeds a force that an approximation's ulp would be lost in)
BEZ_DEV void prox_box(V3 cl, V3 he, const M3& E, V3 r, V3 bc, float& gap, V3& n, V3& p) {
  const float R = (float)BEZ_BALL_RADIUS;
  const V3 ql = mulT(E, bc - r) - cl;
  V3 cp = mk(fminf(fmaxf(ql.x, -he.x), he.x), fminf(fmaxf(ql.y, -he.y), he.y), fminf(fmaxf(ql.z, -he.z), he.z));
  const bool inside = (cp.x == ql.x) && (cp.y == ql.y) && (cp.z == ql.z);
  V3 nl;
  if (!inside) {   // (a NaN centre comes here and is written through)
    const V3 dlt = ql - cp;
    const float dist = sqrtf(dot(dlt, dlt)), inv = 1.f / dist;
    gap = dist - R;
    nl = dlt * inv;
  } else {
    const float dx = he.x - fabsf(ql.x), dy = he.y - fabsf(ql.y), dz = he.z - fabsf(ql.z);
    int ax = 0; float md = dx;
    if (dy < md) { md = dy; ax = 1; }
    if (dz < md) { md = dz; ax = 2; }
    nl = mk(0.f, 0.f, 0.f);
    if (ax == 0) { nl.x = ql.x >= 0.f ? 1.f : -1.f; cp.x = nl.x * he.x; }
    else if (ax == 1) { nl.y = ql.y >= 0.f ? 1.f : -1.f; cp.y = nl.y * he.y; }
    else { nl.z = ql.z >= 0.f ? 1.f : -1.f; cp.z = nl.z * he.z; }
    gap = -(R + md);
  }
  n = mul(E, nl);
  p = r + mul(E, cp + cl);
}
// self_pair's geometry as a signed distance: capsule axes a0-a1, b0-b1 (rel. O), radii ra, rb.  segment_closest is the step's; gap =
// -depth of self_pair, kept when positive; n from b's closest point to a's; p = cb + n (rb - depth / 2), the step's contact point.
BEZ_DEV void prox_pair(float ra, float rb, V3 a0, V3 a1, V3 b0, V3 b1, float& gap, V3& n, V3& p) {
  V3 ca, cb;
  segment_closest(a0, a1, b0, b1, ca, cb);
  const V3 dl = ca - cb;
  const float d2 = dot(dl, dl), rs = ra + rb;
  if (d2 <= 1e-12f) {   // the axes meet: no direction (a NaN is not <=: it goes on and is written through)
    gap = -rs; n = mk(0.f, 0.f, 0.f); p = cb;
    return;
  }
  const float dist = sqrtf(d2), inv = 1.f / dist;
  gap = dist - rs;
  n = dl * inv;
  p = fma3(n, fmaf(0.5f, gap, rb), cb);
}
template <bool CL>
__global__ void __launch_bounds__(PX_THREADS) proximity_kernel(DynArgs D, float* __restrict__ ground, float* __restrict__ ball, float* __restrict__ pairs) {
  __shared__ float frames[PX_TILE * PX_FSTRIDE];
  __shared__ float grows[PX_TILE * PX_GSTRIDE];
  __shared__ float brows[PX_TILE * PX_BSTRIDE];
  __shared__ float prows[PX_TILE * PX_PSTRIDE];
  const int n = D.n, e0 = blockIdx.x * PX_TILE, ne = min(PX_TILE, n - e0);
  if ((int)threadIdx.x < ne) {
    int e = e0 + threadIdx.x;
    float* F = frames + threadIdx.x * PX_FSTRIDE;
    float* G = grows + threadIdx.x * PX_GSTRIDE;
    auto put3 = [&](float* at, V3 v) { at[0] = v.x; at[1] = v.y; at[2] = v.z; };
    const V3 root_pos = state3_at(D, F_ROOT_POS, e), ball_pos = state3_at(D, F_BALL_POS, e);
    const M3 E0 = root_rotation(D, e);
    const float quirk_z = quirk_rz<CL>(D.flags);
    Params P;   // (pt_pos_of looks at the flags alone)
    P.flags = D.flags;
    put3(F + PX_FROOT, root_pos);
    put3(F + PX_FBALL, ball_pos - root_pos);
    put3(G + 3 * BEZ_PROX_BALL_ROW, mk(ball_pos.x, ball_pos.y, ball_pos.z - (float)BEZ_BALL_RADIUS));
    // what link L carries: its ground points (the z word as the step forms it: root_pos.z + x.z), its box's frame, its capsules' axes
    auto link = [&](auto Lk, const M3& E, V3 r) {
      constexpr int L = decltype(Lk)::value;
      static_for<BEZ_NPT>([&](auto I) {
        constexpr int i = decltype(I)::value;
        if constexpr (BEZ_PT_LINK[i] == L) {
          const V3 x = r + mul(E, mk(pt_pos_of<CL>(P, i, 0), pt_pos_of<CL>(P, i, 1), pt_pos_of<CL>(P, i, 2)));
          put3(G + 3 * i, mk(root_pos.x + x.x, root_pos.y + x.y, root_pos.z + x.z));
        }
      });
      if constexpr (link_has_box(L)) {
        float* B = F + PX_FBOX + 12 * link_box(L);
        B[0] = E.m00; B[1] = E.m01; B[2] = E.m02; B[3] = E.m10; B[4] = E.m11; B[5] = E.m12; B[6] = E.m20; B[7] = E.m21; B[8] = E.m22;
        put3(B + 9, r);
      }
      static_for<BEZ_NCAP>([&](auto I) {
        constexpr int c = decltype(I)::value;
        if constexpr (BEZ_CAP_LINK[c] == L) {
          put3(F + PX_FCAP + 6 * c, r + mul(E, mk((float)BEZ_CAP_P0[c][0], (float)BEZ_CAP_P0[c][1], (float)BEZ_CAP_P0[c][2])));
          put3(F + PX_FCAP + 6 * c + 3, r + mul(E, mk((float)BEZ_CAP_P1[c][0], (float)BEZ_CAP_P1[c][1], (float)BEZ_CAP_P1[c][2])));
        }
      });
    };
    link(std::integral_constant<int, 0>{}, E0, mk(0.f, 0.f, 0.f));
    for_each_chain<false>([&](auto first, auto len) {
      asm volatile("" : "+v"(e));   // (opaque per chain, as in inverse_dynamics_kernel)
      M3 E = E0; V3 r = mk(0.f, 0.f, 0.f);
      still_chain_walk<decltype(first)::value, decltype(len)::value>(E, r, quirk_z, [&](auto Lk) { return state_at(D, F_Q + decltype(Lk)::value - 1, e); },
                                                                     [&](auto Lk, const SV&) { link(Lk, E, r); });
    });
  }
  __syncthreads();
  const bool box_asset = (D.flags & BEZ_FLAG_BOX_ASSET) != 0;
  const int first = pairs ? 0 : PX_TILE * BEZ_NCPAIR, last = ball ? PX_TILE * (BEZ_NCPAIR + BEZ_NBOX) : PX_TILE * BEZ_NCPAIR;
  for (int i = first + threadIdx.x; i < last; i += PX_THREADS) {
    const int el = i % PX_TILE, t = i / PX_TILE;
    if (el >= ne) continue;
    const float* F = frames + el * PX_FSTRIDE;
    float gap; V3 nn, p;
    if (t < BEZ_NCPAIR) {
      const int ia = PROX_TABLES.pair[t][0], ib = PROX_TABLES.pair[t][1];
      const float *A = F + PX_FCAP + 6 * ia, *B = F + PX_FCAP + 6 * ib;
      prox_pair(PROX_TABLES.cap_r[ia], PROX_TABLES.cap_r[ib], lds3(A), lds3(A + 3), lds3(B), lds3(B + 3), gap, nn, p);
      prox_put(prows + el * PX_PSTRIDE + BEZ_PROX_WORDS * t, gap, nn, p, lds3(F + PX_FROOT));
    } else {
      const int b = t - BEZ_NCPAIR, k = (b == BEZ_TORSO_BOX && box_asset) ? BEZ_NBOX : b;
      const float* B = F + PX_FBOX + 12 * b;
      const M3 E = {B[0], B[1], B[2], B[3], B[4], B[5], B[6], B[7], B[8]};
      prox_box(lds3(PROX_TABLES.center[k]), lds3(PROX_TABLES.half[k]), E, lds3(B + 9), lds3(F + PX_FBALL), gap, nn, p);
      prox_put(brows + el * PX_BSTRIDE + BEZ_PROX_WORDS * b, gap, nn, p, lds3(F + PX_FROOT));
    }
  }
  __syncthreads();
  if (ground) tile_store<PX_GW, PX_GSTRIDE, PX_THREADS>(grows, ground + (size_t)e0 * PX_GW, ne);
  if (ball) tile_store<PX_BW, PX_BSTRIDE, PX_THREADS>(brows, ball + (size_t)e0 * PX_BW, ne);
  if (pairs) tile_store<PX_PW, PX_PSTRIDE, PX_THREADS>(prows, pairs + (size_t)e0 * PX_PW, ne);
}

// ---- bez_sim_apply_body_forces: one thread per env turns the Isaac-layout inputs of its env into the pending per-link wrenches (bez_kernels.h
// ext_wrench): forward kinematics of the current state for the link frames, LOCAL vectors and every point of application resolved now,
// fixed bodies folded into their links, everything ADDED to what earlier calls left (read-modify-write by the env's one thread).
template <bool CL>
__global__ void ext_prepare_kernel(const float* __restrict__ st, float* __restrict__ ext, const float* __restrict__ F, const float* __restrict__ T,
                                   const float* __restrict__ X, int local, int n, int has_ball, uint32_t flags) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  EnvState S;
  load_state(st, n, e, S);
  M3 E[BEZ_NL]; V3 r[BEZ_NL]; SV V[BEZ_NL];
  link_frames<CL, false>(S, flags, E, r, V);
  constexpr int NB = nb_of<CL>();
  const int nbe = NB + (has_ball ? 1 : 0);
  bool any = false;
  // adds (force fw, torque tw, point p in the frame of link l) to link l's entries
  auto add = [&](int l, V3 fw, V3 tw, V3 p) {
    float* x = ext + (size_t)l * EXT_COMP * n + e;
    const float v[EXT_COMP] = {fw.x, fw.y, fw.z, tw.x, tw.y, tw.z, p.x * fw.x, p.x * fw.y, p.x * fw.z, p.y * fw.x, p.y * fw.y, p.y * fw.z,
                               p.z * fw.x, p.z * fw.y, p.z * fw.z};
#pragma unroll
    for (int k = 0; k < EXT_COMP; ++k) x[(size_t)k * n] += v[k];
  };
  auto in3 = [&](const float* a, int b) { const float* q = a + ((size_t)e * nbe + b) * 3; return mk(q[0], q[1], q[2]); };
  for (int b = 0; b < nbe; ++b) {
    const V3 f = F ? in3(F, b) : mk(0, 0, 0), t = T ? in3(T, b) : mk(0, 0, 0);
    if (!(f.x != 0.f || f.y != 0.f || f.z != 0.f || t.x != 0.f || t.y != 0.f || t.z != 0.f)) continue;   // (a NaN is != 0: it goes in)
    any = true;
    if (b < NB) {   // a robot body: its link's frame, its origin's offset in that frame, its own centre of mass
      const BodyFrame bf = body_frame<CL>(b);
      const int l = bf.link;
      V3 p;
      if (!X) p = bf.off + bf.com;
      else if (local) p = bf.off + in3(X, b);
      else p = mulT(E[l], in3(X, b) - S.root_pos - r[l]);
      add(l, local ? mul(E[l], f) : f, local ? mul(E[l], t) : t, p);
    } else {        // the ball: its own frame about its centre
      const M3 Rb = quat_to_mat(S.bq[0], S.bq[1], S.bq[2], S.bq[3]);
      const V3 p = !X ? mk(0, 0, 0) : (local ? in3(X, b) : mulT(Rb, in3(X, b) - S.ball_pos));
      add(BEZ_NL, local ? mul(Rb, f) : f, local ? mul(Rb, t) : t, p);
    }
  }
  if (any) ext[(size_t)EXT_FLAG * n + e] = 1.f;
}

}  // namespace bez
