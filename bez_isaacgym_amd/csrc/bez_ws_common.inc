// bez_ws_common.inc -- building blocks of the wave-specialised kernel (bez_kernel_ws8.h: 8 role waves; kept apart from the role
// schedule).  Included INSIDE the kernel's namespace after it has defined its LDS slot map (X_* enum incl. X_STAGE), WS_ENVS,
// the joint ownership of its roles (role_ndof / role_dof) and its split of the leg<->leg pairs (self_part_owns / self_fk_depth).
#define XS(slot) lds[(slot) * WS_LANES + lane]

// Workgroup barrier for data exchanged through LDS only (nothing a role writes to global memory is read by another role in the
// same launch): waits for this wave's LDS traffic, NOT for its outstanding global loads / stores as __syncthreads() does
// (s_waitcnt vmcnt(0)) -- the state stores of the post-physics and the prefetched rows stay in flight across it.
BEZ_DEV void ws_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// In-kernel stamps (diagnostic build only; the shipped one-lane kernel contains none, the lane-group form keeps their branches: below): clock at phase boundaries of
// workgroup 0, written to a buffer nothing else reads.
#ifdef BEZ_WS_STAMPS
#define WS_STAMP(role, k)                                                                         \
  do {                                                                                            \
    if (P.stamps && blockIdx.x == 0 && lane == 0) P.stamps[(role) * 32 + (k)] = __builtin_amdgcn_s_memtime(); \
  } while (0)
#elif BEZ_WS_SUB == 4
// The lane-group form keeps the stamps' BRANCHES (never taken: P.stamps is null outside the diagnostic build).  Each is a basic-block
// boundary at a phase boundary, and the compiler's scheduler does not move one phase's arithmetic into the next across it.  Found because
// the diagnostic build of this form was FASTER than the build without them; measured on one box (tools/ab_bench.py, full stores):
// none 26.1 us, all 23.9, all but the root role's 26.2, only the root role's 24.4, per joint of pass 2 as well 24.5; of the root role's
// fifteen, the one behind B0 and the one behind B2 carry the gain (BEZ_WS_ROOT_MASK 0x42: 23.6 us; with all fifteen the root role
// alone spills 18 VGPRs).  In the one-lane form the same branches cost 1 us (28.8 against 27.8): it keeps none.
#define WS_STAMP(role, k)                                       \
  do {                                                          \
    if (P.stamps) asm volatile("s_nop 0" ::: "memory");         \
  } while (0)
#else
#define WS_STAMP(role, k) do { } while (0)
#endif
// the root role's stamps, numbered in program order: BEZ_WS_ROOT_MASK selects which of them stay as fences in the lane-group form
#ifndef BEZ_WS_ROOT_MASK
#define BEZ_WS_ROOT_MASK 0x0042
#endif
#ifdef BEZ_WS_STAMPS
#define WS_STAMP_ROOT_N(n, role, k) WS_STAMP(role, k)
#else
#define WS_STAMP_ROOT_N(n, role, k) do { if constexpr (((BEZ_WS_ROOT_MASK) >> (n)) & 1) { WS_STAMP(role, k); } } while (0)
#endif

BEZ_DEV void xs_store_sv(float* lds, int lane, int slot, SV v) {
  XS(slot + 0) = v.a.x; XS(slot + 1) = v.a.y; XS(slot + 2) = v.a.z; XS(slot + 3) = v.l.x; XS(slot + 4) = v.l.y; XS(slot + 5) = v.l.z;
}
BEZ_DEV SV xs_load_sv(const float* lds, int lane, int slot) {
  return mksv(mk(XS(slot + 0), XS(slot + 1), XS(slot + 2)), mk(XS(slot + 3), XS(slot + 4), XS(slot + 5)));
}
BEZ_DEV void xs_store_v3(float* lds, int lane, int slot, V3 v) { XS(slot) = v.x; XS(slot + 1) = v.y; XS(slot + 2) = v.z; }
BEZ_DEV V3 xs_load_v3(const float* lds, int lane, int slot) { return mk(XS(slot), XS(slot + 1), XS(slot + 2)); }
BEZ_DEV void xs_store_sym6(float* lds, int lane, int slot, const Sym6& I, SV p) {
  const float* f = (const float*)&I;
#pragma unroll
  for (int i = 0; i < 21; ++i) XS(slot + i) = f[i];
  xs_store_sv(lds, lane, slot + 21, p);
}
BEZ_DEV void xs_add_sym6(const float* lds, int lane, int slot, Sym6& I, SV& p) {
  float* f = (float*)&I;
#pragma unroll
  for (int i = 0; i < 21; ++i) f[i] += XS(slot + i);
  p = p + xs_load_sv(lds, lane, slot + 21);
}
// net-contact-force row of `body`: the first contributing substep stores w * f, later ones add (cf_accum of bez_kernels.h, in LDS)
BEZ_DEV void ws_cf_acc(float* lds, int lane, int body, V3 f, float w, bool first) {
  const int s = X_CF + body * 3;
  if (first) { XS(s) = f.x * w; XS(s + 1) = f.y * w; XS(s + 2) = f.z * w; }
  else { XS(s) = fmaf(f.x, w, XS(s)); XS(s + 1) = fmaf(f.y, w, XS(s + 1)); XS(s + 2) = fmaf(f.z, w, XS(s + 2)); }
}
// the two helper parts' leg<->leg contact results of leg box link k (see ws_self_collision)
BEZ_DEV SV xs_self_wrench(const float* lds, int lane, int k) { return xs_load_sv(lds, lane, X_SELF + k * 9) + xs_load_sv(lds, lane, X_SELF + 90 + k * 9); }
BEZ_DEV V3 xs_self_force(const float* lds, int lane, int k) { return xs_load_v3(lds, lane, X_SELF + k * 9 + 6) + xs_load_v3(lds, lane, X_SELF + 90 + k * 9 + 6); }
// leg box link L (6..10 / 14..18) -> 0..9
BEZ_DEV constexpr int self_index(int L) { return L < 11 ? L - 6 : 5 + (L - 14); }

// shared (read-only within a substep) root / ball state as the chain roles see it
struct RootView { M3 E0; SV V0; float root_z; V3 bc, ball_lin, ball_ang; float ball_z; };
BEZ_DEV RootView load_root_view(const float* lds, int lane) {
  RootView R;
  V3 pos = xs_load_v3(lds, lane, X_ROOT);
  R.E0 = quat_to_mat(XS(X_ROOT + 3), XS(X_ROOT + 4), XS(X_ROOT + 5), XS(X_ROOT + 6));
  R.V0 = mksv(xs_load_v3(lds, lane, X_ROOT + 10), xs_load_v3(lds, lane, X_ROOT + 7));
  R.root_z = pos.z;
  V3 bp = xs_load_v3(lds, lane, X_BALL);
  R.bc = bp - pos; R.ball_z = bp.z;
  R.ball_lin = xs_load_v3(lds, lane, X_BALL + 3); R.ball_ang = xs_load_v3(lds, lane, X_BALL + 6);
  return R;
}

// keeps a value (and the instructions that produce it) where it is written: an empty asm the compiler cannot move code across
BEZ_DEV void pin(float& x) { asm volatile("" : "+v"(x)); }
BEZ_DEV void pin(V3& v) { pin(v.x); pin(v.y); pin(v.z); }
// per-joint data a chain keeps in registers between pass 2 and pass 3.
// DF, the actuator record (bez_kernels.h df_record): a speed-limit-locked joint (1/D = 0: UD would hold zeros) keeps U itself in UD -- every
// use for the dynamics reads it as zero -- and c0 = S.pA + U.c + (J + armature) qdd, the part of its reaction that pass 2 knows; the
// chain's decision bits travel in one word (DfWord: four bits per joint)
template <bool DF> struct P3 { SV UD; float uD, Dinv; SV S, cb; };
template <> struct P3<true> { SV UD; float uD, Dinv; SV S, cb; float c0; };
// contact rows of a body: F = F0 - (B^T a_ang + C a_lin) for the body's spatial acceleration a
struct BodyContact { M3 B; Sym3 C; V3 F0; };
BEZ_DEV BodyContact body_contact_of(const Sym6& Kc, SV pc) { BodyContact b; b.B = Kc.B; b.C = Kc.C; b.F0 = -pc.l; return b; }
BEZ_DEV V3 body_contact_force(const BodyContact& b, SV a) { return b.F0 - (mulT(b.B, a.a) + mul(b.C, a.l)); }

// `hits` != null (cleats asset, foot links): the per-point records are kept in LDS, every cleat reports its own contact row
template <int L, bool CL>
BEZ_DEV void ws_ground_points(const Params& P, float mu, float root_z, const M3& E, V3 r, SV V, Sym6& Kc, SV& pc, float* lds = nullptr, int lane = 0, int hit0 = 0) {
  int k = 0;
#pragma unroll
  for (int i = 0; i < BEZ_NPT; ++i) {
    if (BEZ_PT_LINK[i] == L) {
      V3 pl = mk(pt_pos_of<CL>(P, i, 0), pt_pos_of<CL>(P, i, 1), pt_pos_of<CL>(P, i, 2));
      V3 x = r + mul(E, pl);
      Hit h = ground_contact(P, P.kn, P.cn, mu, x, root_z + x.z, V, Kc, pc);
      if (CL && lds) {
        const int s0 = hit0 + k * 8;
        XS(s0) = h.x.x; XS(s0 + 1) = h.x.y; XS(s0 + 2) = h.x.z; XS(s0 + 3) = h.fn0; XS(s0 + 4) = h.kn; XS(s0 + 5) = h.ct; XS(s0 + 6) = h.ftx0; XS(s0 + 7) = h.fty0;
      }
      ++k;
    }
  }
}
// the cleat rows of one foot from the records above and the foot's acceleration
template <int L>
BEZ_DEV void ws_cleat_forces(const Params& P, float* lds, int lane, int hit0, SV a, bool first) {
  int k = 0;
#pragma unroll
  for (int i = 0; i < BEZ_NPT; ++i) {
    if (BEZ_PT_LINK[i] == L) {
      const int s0 = hit0 + k * 8;
      Hit h; h.x = mk(XS(s0), XS(s0 + 1), XS(s0 + 2)); h.fn0 = XS(s0 + 3); h.kn = XS(s0 + 4); h.ct = XS(s0 + 5); h.ftx0 = XS(s0 + 6); h.fty0 = XS(s0 + 7);
      V3 f = h.kn > 0.f ? cf_ground(P, hit_force(P, h, a)) : mk(0, 0, 0);
      ws_cf_acc(lds, lane, BEZ_PT_BODY_CL[i], f, P.cf_w, first);
      ++k;
    }
  }
}

// Per-role DR scalars
struct ChainDyn { float mu; V3 g; };

// ---- passes 1+2 of one serial chain.  Outputs the chain's articulated inertia/bias as seen by the torso (added to
// IAo/pAo), the pass-3 operands p3[LEN], the contact rows of the chain-end link, and (legs) the ball/box candidate.
// BAR_AFTER >= 0: a workgroup barrier is executed after that link when `bar` is set (the 8-wave kernel's deferred ball update
// meets the other roles there)
// EXT: `xp` = env e has external wrenches pending (bez_sim_apply_body_forces): each link's enters its bias force here, in every substep
template <int FIRST, int LEN, bool LEG, bool CL, bool BOX = LEG, int BAR_AFTER = -1, bool EXT = false>
BEZ_DEV void ws_chain_pass1(const Params& P, const ChainDyn& D, const float* ms, const RootView& R, const float* q, const float* qd,
                            LinkInertia* LI, SV* pAl, SV* Sl, SV* cbl, M3& Eend, V3& rend, SV& Vend, BallSel& sel, SV& Vsel, bool bar = false,
                            int e = 0, bool xp = false) {
  M3 E = R.E0;
  V3 r = mk(0, 0, 0);
  SV V = R.V0;
  static_for<LEN>([&](auto I) {
    constexpr int i = decltype(I)::value;
    constexpr int L = FIRST + i;
    link_kinematics<L>(q[i], qd[i], E, r, V, Sl[i], cbl[i], quirk_rz<CL>(P.flags));
    link_inertia<L, CL>(ms[i], D.g, E, r, V, LI[i], pAl[i]);
    if constexpr (EXT) { if (xp) pAl[i] = pAl[i] - ext_wrench(P, e, L, E, r); }
    if constexpr (i == BAR_AFTER) { if (bar) ws_barrier(); }
    if constexpr (BOX && link_has_box(L)) {
      test_box<link_box(L)>(E, r, R.bc, sel);
      if (sel.link == L) Vsel = V;  // this box just became the deepest candidate: keep its link velocity
    }
  });
  Eend = E; rend = r; Vend = V;  // chain-end frame / velocity for the ground points
}

template <bool DF, int FIRST, int LEN, bool LEG>
BEZ_DEV void ws_chain_pass2(const Params& P, const ChainDyn& D, const float* kps, const float* kds, const float* lo, const float* hi,
                            const float* q, const float* qd, const float* target, const LinkInertia* LI, const SV* pAl, const SV* Sl,
                            const SV* cbl, const Sym6& Kc, SV pc, bool mine, BallSel& sel, P3<DF>* p3, Sym6& IAo, SV& pAo, DfWord<DF>& dfw) {
  Sym6 IA = Kc;
  SV pA = pc;
  static_for<LEN>([&](auto I) {
    constexpr int i = LEN - 1 - decltype(I)::value;
    constexpr int L = FIRST + i;
    add_link_inertia(IA, LI[i]);
    pA = pA + pAl[i];
    if constexpr (LEG && link_has_box(L)) {
      if (mine && sel.link == L) {  // contact operands were prepared once, by the root role (X_FOLD)
        add_point_stiffness(IA, sel.x, sel.A);
        pA = pA - wrench_at(sel.x, sel.f0p);
      }
    }
    SV U; float Dinv, uD, qhp;
    DfJoint<DF> df;
    joint_terms<L>(P, kps[i], kds[i], lo[i], hi[i], q[i], qd[i], target[i], IA, pA, Sl[i], cbl[i], U, Dinv, uD, qhp, 0.f, 0.f, df);   // (a speed-limited joint: Dinv = 0, uD = its prescribed acceleration)
    if constexpr (DF) dfw.w |= df.bits << (4 * i);
    // p3.uD keeps the HELD-PARENT acceleration qhp = uD - (U/D).c: pass 3 then needs no c in its dot product (qdd = qhp - (U/D).a_parent),
    // and the leg<->leg scale reads it as it is
    p3[i].UD = U * Dinv; p3[i].uD = qhp; p3[i].Dinv = Dinv; p3[i].S = Sl[i]; p3[i].cb = cbl[i];
    if constexpr (DF) {
      if (df.bits & DF_LOCK) p3[i].UD = U;
      p3[i].c0 = df.c0 + dot(U, cbl[i]);
    }
    add_outer(IA, U, -Dinv);
    pA = pA + mul(IA, cbl[i]) + U * uD;
#ifdef BEZ_WS_STAMPS
    if constexpr (LEG && FIRST == 5) { const int lane = threadIdx.x & 63; pin(pA.a); pin(pA.l); WS_STAMP(0, 26 + i); }  // per-joint progress of the left leg (last substep)
#endif
  });
  add_to(IAo, IA);
  pAo = pAo + pA;
}

// The leg<->leg contact wrenches enter AFTER pass 2 (the helper waves compute them while the legs run passes 1-2): an extra bias
// force dp on link i changes u_i by -S_i . dp and travels up the chain as (1 - U_i S_i^T / D_i) dp, an exact linear correction of
// pass 2's bias recursion (the predictors do not see these forces: same rule in the oracle).  Round 6: every pair force of the env is
// scaled by ONE factor sc that stands for the contact's implicit part (oracle: self_contact_scale); it needs two sums over BOTH
// legs' joints (and the pairs' sum of |force|^2, which the helper parts leave in X_SELFF2).  The two leg waves exchange their partial sums between themselves (X_SELFSUM aliases the pose-error slots, which are
// only written after the last substep): each runs the correction recursion on the unscaled wrenches, publishes its two
// numbers and a sequence word, and waits for the other leg's word (the legs run the same code side by side: the wait is short).  No workgroup barrier is
// spent on it, and nothing is added to the root role (at the register ceiling: the scale's six loads and a division there cost 31
// spilled VGPRs and 3 us per step when round 6 first put them there).
// (the words are accessed through an explicit LDS pointer: a volatile access through the generic `float*` the helpers pass around compiles
// to flat_load / flat_store with system-scope cache control and a full `s_waitcnt vmcnt(0)` -- 2 us per step when round 6 first had it so)
typedef __attribute__((address_space(3))) volatile int lds_word_t;
BEZ_DEV void ws_pair_publish(float* lds, int side, int seq) {
  // this wave's LDS stores above are complete before the word that announces them (LDS serves a wave's requests in order; the wait makes it explicit)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  lds_word_t* flag = (lds_word_t*)(lds + X_PAIRSEQ * WS_LANES);
  flag[side] = seq;
}
// a bounded hand-over wait that gave up: the step goes on with stale words, and says so -- a word in LDS (lane 4 of the X_PAIRSEQ slot,
// zeroed at kernel entry), turned into BEZ_HEALTH_SPIN_TIMEOUT in the health word by one copy-out thread behind the last barrier
BEZ_DEV void ws_spin_timeout(const float* lds) { ((lds_word_t*)(lds + X_PAIRSEQ * WS_LANES))[4] = 1; }
// EXIT_IN_LOOP: where the timeout is noticed -- at the bound inside the loop, or by a second read behind it.  The two compile to the same
// waits; the cleats kernels keep their register budget with the first, the others with the second (tools/kernel_resources.sh).
template <bool EXIT_IN_LOOP>
BEZ_DEV void ws_pair_wait(const float* lds, int side, int seq) {
  lds_word_t* flag = (lds_word_t*)(lds + X_PAIRSEQ * WS_LANES);
  // bounded: a wave that never arrives would be a bug, not a reason to hang the GPU (the bound is ~10^3 times the longest wait seen)
  if constexpr (EXIT_IN_LOOP) {
#pragma unroll 1
    for (int guard = 0; flag[1 - side] < seq; ++guard) {
      if (guard == (1 << 16)) { ws_spin_timeout(lds); break; }
      __builtin_amdgcn_s_sleep(1);
    }
  } else {
#pragma unroll 1
    for (int guard = 0; guard < (1 << 16) && flag[1 - side] < seq; ++guard) __builtin_amdgcn_s_sleep(1);
    if (flag[1 - side] < seq) ws_spin_timeout(lds);   // still missing after the bound
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}
template <bool DF, int LEN, bool CL>
BEZ_DEV float ws_chain_self_correction(const Params& P, float* lds, int lane, int side, int seq, P3<DF>* p3, SV& pAo, DfWord<DF> dfw) {
  static_assert(LEN == 6, "legs only");
  SV w[LEN];  // all wrenches are fetched up front (one burst of LDS reads): the chain below is serial and would expose each latency
  static_for<LEN>([&](auto I) {
    constexpr int i = decltype(I)::value;
    if constexpr (i >= 1) w[i] = xs_self_wrench(lds, lane, side * 5 + i - 1);
  });
  static_for<LEN>([&](auto I) {
    constexpr int i = decltype(I)::value;
    if constexpr (i >= 1) { pin(w[i].a); pin(w[i].l); }
  });
  // one sweep: this leg's share of the two joint sums -- the contacts' generalised force on each joint (minus: the slots hold bias
  // forces) against the joint's held-parent acceleration (p3.uD holds it: see ws_chain_pass2) and its 1/D -- and the correction
  // recursion on the unscaled wrenches
  SV acc = svzero(), wsub = svzero();
  float am = 0.f, as = 0.f;
  static_for<LEN>([&](auto I) {
    constexpr int i = LEN - 1 - decltype(I)::value;
    if constexpr (i >= 1) { acc = acc + w[i]; wsub = wsub + w[i]; }
    const float tq = dot(p3[i].S, wsub);
    as = fmaf(tq * tq, p3[i].Dinv, as); am = fmaf(-tq, p3[i].uD, am);
    const float sd = -dot(p3[i].S, acc);
    if constexpr (DF) {
      const bool lk = ((dfw.w >> (4 * i)) & DF_LOCK) != 0u;   // locked: UD holds U (read as zero here); Dinv keeps sd = -S.(the contacts' bias) for the reaction
      acc = acc + p3[i].UD * (lk ? 0.f : sd);
      p3[i].Dinv = lk ? sd : sd * p3[i].Dinv;
    } else {
      acc = acc + p3[i].UD * sd;
      p3[i].Dinv = sd * p3[i].Dinv;   // from here on: the contacts' unscaled share of this joint's acceleration
    }
  });
  XS(X_SELFSUM + side * 2) = am; XS(X_SELFSUM + side * 2 + 1) = as;
  ws_pair_publish(lds, side, seq);
  ws_pair_wait<CL>(lds, side, seq);
  SelfSums Z;
  Z.am = XS(X_SELFSUM) + XS(X_SELFSUM + 2); Z.as = XS(X_SELFSUM + 1) + XS(X_SELFSUM + 3); Z.f2 = XS(X_SELFF2) + XS(X_SELFF2 + 1);   // (the helper parts' sums of |force|^2)
  const float sc = self_scale(P, Z);
#pragma unroll
  for (int i = 0; i < LEN; ++i) {
    if constexpr (DF) {
      const bool lk = ((dfw.w >> (4 * i)) & DF_LOCK) != 0u;
      p3[i].uD = fmaf(sc, lk ? 0.f : p3[i].Dinv, p3[i].uD);
      p3[i].c0 = lk ? fmaf(-sc, p3[i].Dinv, p3[i].c0) : p3[i].c0;
    } else {
      p3[i].uD = fmaf(sc, p3[i].Dinv, p3[i].uD);
    }
  }
  pAo = pAo + acc * sc;
  xs_store_sv(lds, lane, X_IA + side * 27 + 21, pAo);
  return sc;
}

// pass 3: joint accelerations, semi-implicit Euler (the speed limit is inside the dynamics: joint_terms); returns the chain-end acceleration.
// sc = the leg<->leg contacts' common scale (their reported forces carry it too).  dfw, the gains, limits and targets, e, sub (the substep's
// index) and active (the lane owns env e's stores): read by the actuator record only
template <bool DF, int FIRST, int LEN, bool LEG, bool CL>
BEZ_DEV SV ws_chain_pass3(const Params& P, SV a0, const P3<DF>* p3, float* q, float* qd, bool mine, const BallSel& sel, V3& fl, V3& f_end,
                          float* lds, int lane, bool keep, bool first, float sc, DfWord<DF> dfw, const float* kps, const float* kds, const float* lo,
                          const float* hi, const float* target, int e, int sub, bool active) {
  SV a = a0;
  static_for<LEN>([&](auto I) {
    constexpr int i = decltype(I)::value;
    constexpr int L = FIRST + i;
    float qdd;
    if constexpr (DF) {
      const uint32_t dfb = (dfw.w >> (4 * i)) & 15u;
      const float dUa = dot(p3[i].UD, a);   // a locked joint's UD holds U: U.a_parent, the rest of its reaction
      qdd = (dfb & DF_LOCK) ? p3[i].uD : p3[i].uD - dUa;
      if (active) df_record(P, e, sub, L - 1, dfb, kps[i], kds[i], lo[i], hi[i], q[i], qd[i], target[i], qdd, p3[i].c0 + dUa);
    } else {
      qdd = p3[i].uD - dot(p3[i].UD, a);   // (p3.uD = the held-parent acceleration: the bias acceleration c is already in it)
    }
    a = a + p3[i].cb + p3[i].S * qdd;
    float v = fmaf(P.h, qdd, qd[i]);
    qd[i] = v;
    q[i] = fmaf(P.h, v, q[i]);
    if constexpr (LEG && link_has_box(L)) {
      V3 f = xs_self_force(lds, lane, self_index(L)) * sc;  // leg<->leg contacts of this link
      if (mine && sel.link == L) { fl = sel.f0p - mul(sel.A, point_of(a, sel.x)); f = f + cf_along(P, fl, sel.n); }
      if (keep) {
        if constexpr (i == LEN - 1) f_end = f;
        else ws_cf_acc(lds, lane, link_body<CL>(L), f, P.cf_w, first);
      }
    }
  });
  return a;
}

// ---- joint-side post-physics of a chain role (runs in parallel in the three chain waves): the reset draw for ITS joints
// (kick_env.py:786-791,839-842), the observation slots q / qd (kick_env.py:1409-1410), its share of |default - q|^2, and
// the stores of its joints' state.
BEZ_DEV constexpr bool role_needs_block(int role, int b) {
  for (int i = 0; i < role_ndof(role); ++i) if ((role_dof(role, i) >> 2) == b || ((BEZ_ND + role_dof(role, i)) >> 2) == b) return true;
  return false;
}
template <int ROLE, bool POST>
BEZ_DEV void ws_chain_epilogue(const Params& P, float* lds, int lane, int e, bool active, bool do_reset, uint32_t episode,
                               float* q, float* qd, float* target) {
  const int n = P.n;
  asm volatile("" : "+v"(e));  // the store addresses below are formed HERE, not hoisted to the kernel entry and carried (64-bit) through the physics
  bool bad = false;             // the non-finite guard tripped on this role's joints
  if (POST) {
    if (do_reset) {
      const int64_t genv = P.env_off + e;
      const uint32_t k0 = (uint32_t)P.seed, k1 = (uint32_t)(P.seed >> 32);
      static_for<9>([&](auto B) {
        constexpr int b = decltype(B)::value;
        if constexpr (role_needs_block(ROLE, b)) {
          uint32_t c[4] = {(uint32_t)genv, (uint32_t)((uint64_t)genv >> 32), episode, (uint32_t)b};
          philox4x32_10(c, k0, k1);
          static_for<role_ndof(ROLE)>([&](auto I) {
            constexpr int i = decltype(I)::value;
            constexpr int d = role_dof(ROLE, i);
            if constexpr ((d >> 2) == b) {
              float u = (float)(c[d & 3] >> 8) * (1.0f / 16777216.0f);
              float qq = (float)BEZ_DOF_DEFAULT[d] + fmaf(0.3f, u, -0.15f);
              q[i] = fmaxf(fminf(qq, (float)BEZ_DOF_UPPER[d]), (float)BEZ_DOF_LOWER[d]);
            }
            if constexpr (((BEZ_ND + d) >> 2) == b) {
              float u = (float)(c[(BEZ_ND + d) & 3] >> 8) * (1.0f / 16777216.0f);
              qd[i] = fmaf(0.2f, u, -0.1f);
            }
          });
        }
      });
      static_for<role_ndof(ROLE)>([&](auto I) { constexpr int i = decltype(I)::value; target[i] = (float)BEZ_DOF_DEFAULT[role_dof(ROLE, i)]; });
    }
    float* obs_row = lds + X_STAGE * WS_LANES + ws_env_of(lane) * P.nobs;
    float psum = 0.f;
    static_for<role_ndof(ROLE)>([&](auto I) {
      constexpr int i = decltype(I)::value;
      constexpr int d = role_dof(ROLE, i);
      obs_row[d] = q[i]; obs_row[BEZ_ND + d] = qd[i];
      float dd = (float)BEZ_DOF_DEFAULT[d] - q[i];
      psum = fmaf(dd, dd, psum);
    });
    // the non-finite guard: psum is non-finite when a q is (or overflows); the velocities are checked through their sum.  A bad joint
    // publishes a NaN pose-error share (the root role reads the trip from it behind the last barrier) and takes the cold re-store below.
    if (guard_on(P)) {
      float vs = 0.f;
      static_for<role_ndof(ROLE)>([&](auto I) { vs += qd[decltype(I)::value]; });
      bad = nonfinite(psum) | nonfinite(vs);
      if (bad) psum = __builtin_nanf("");
    }
    XS(X_PSUM + ROLE) = psum;
  }
  if (active) {
    float* st = P.state;
    static_for<role_ndof(ROLE)>([&](auto I) {
      constexpr int i = decltype(I)::value;
      constexpr int d = role_dof(ROLE, i);
      st[(size_t)(F_Q + d) * n + e] = q[i]; st[(size_t)(F_QD + d) * n + e] = qd[i]; st[(size_t)(F_TARGET + d) * n + e] = target[i];
    });
    if (bad) {   // cold: the non-finite values again, as their replacements (default position, zero velocity); same lane, program order
      static_for<role_ndof(ROLE)>([&](auto I) {
        constexpr int i = decltype(I)::value;
        constexpr int d = role_dof(ROLE, i);
        if (nonfinite(q[i])) st[(size_t)(F_Q + d) * n + e] = (float)BEZ_DOF_DEFAULT[d];
        if (nonfinite(qd[i])) st[(size_t)(F_QD + d) * n + e] = 0.f;
      });
    }
  }
}

// ---- leg<->leg self-collision, evaluated by the two waves that would otherwise idle while the leg roles run pass 1:
// PART 0 (upper role, in the window of the legs' pass 1) owns the hip/thigh x hip/thigh pairs and only walks both legs down to
// the thigh; PART 1 (root role, in the window of the legs' pass 2) owns every other pair of BEZ_CPAIR.  Forward kinematics of both legs comes from the joint state
// the leg roles published (X_LEGQ); per-link wrenches / reported forces are summed in registers and written once to this
// part's LDS block (X_SELF + PART * 90: link k -> wrench 6 floats at k*9, force 3 floats at k*9+6); the legs add both blocks.
struct SelfCaps { V3 c0[BEZ_NCAP], c1[BEZ_NCAP]; SV V[BEZ_NCAP]; };  // world end points / link velocity per capsule (left 0..5, right 6..11)
// stage 1: forward kinematics of both legs (as deep as this part's pairs need) -> capsules
#if BEZ_WS_SUB == 4
template <int L> BEZ_DEV void wq_store_package(float* lds, int lane, int side, int i, V3 g, const M3& E, V3 r, SV V);   // bez_ws_quad.inc
#endif
// PKG_SIDE >= 0 (lane-group form, default asset): the packages of that leg's ankle and foot links are left in LDS for the leg role on the
// way (bez_ws_quad.inc: wq_store_package)
template <int PART, int BAR_AFTER = -1, int PKG_SIDE = -1>
BEZ_DEV void ws_self_fk(float* lds, int lane, const M3& E0, SV V0, SelfCaps& K, bool bar = false, float quirk_z = BEZ_QUIRK_RZ, V3 g = V3{0.f, 0.f, 0.f}) {
  static_for<2>([&](auto SIDE) {
    constexpr int side = decltype(SIDE)::value;
    constexpr int NFK = self_fk_depth(PART, side);  // links to walk down this leg
    M3 E = E0; V3 r = mk(0, 0, 0); SV V = V0, Sj, cbj;
    static_for<NFK>([&](auto I) {
      constexpr int i = decltype(I)::value;
      constexpr int L = (side == 0 ? 5 : 13) + i;
      link_kinematics<L>(XS(X_LEGQ + side * 12 + i), XS(X_LEGQ + side * 12 + 6 + i), E, r, V, Sj, cbj, quirk_z);
      static_for<BEZ_NCAP>([&](auto C) {
        constexpr int c = decltype(C)::value;
        if constexpr (BEZ_CAP_LINK[c] == L) {
          K.c0[c] = r + mul(E, mk((float)BEZ_CAP_P0[c][0], (float)BEZ_CAP_P0[c][1], (float)BEZ_CAP_P0[c][2]));
          K.c1[c] = r + mul(E, mk((float)BEZ_CAP_P1[c][0], (float)BEZ_CAP_P1[c][1], (float)BEZ_CAP_P1[c][2]));
          K.V[c] = V;
        }
      });
#if BEZ_WS_SUB == 4
      if constexpr (side == PKG_SIDE && i >= 4) wq_store_package<L>(lds, lane, side, i, g, E, r, V);
#endif
      if constexpr (side == 0 && i == BAR_AFTER) { if (bar) ws_barrier(); }  // 8-wave kernel: the deferred B5 of the previous substep
    });
  });
}
// Keeps stage 1 where it is written: without this the compiler sinks the kinematics past the barriers to their first use,
// i.e. out of the idle window they are meant to fill.
template <int PART>
BEZ_DEV void ws_self_pin(SelfCaps& K) {
  static_for<BEZ_NCAP>([&](auto C) {
    constexpr int c = decltype(C)::value;
    constexpr int depth = BEZ_CAP_LINK[c] < 11 ? BEZ_CAP_LINK[c] - 5 : BEZ_CAP_LINK[c] - 13;
    if constexpr (depth < self_fk_depth(PART, c < BEZ_NCAP / 2 ? 0 : 1)) { pin(K.c0[c]); pin(K.c1[c]); pin(K.V[c].a); pin(K.V[c].l); }
  });
}
// stage 2: this part's capsule pairs -> per-link wrench / reported force, one LDS block per part
template <int PART>
BEZ_DEV void ws_self_pairs(const Params& P, float mu, float* lds, int lane, const SelfCaps& K) {
  constexpr int base = X_SELF + PART * 90;
  SV w[10]; V3 cf[10]; float f2 = 0.f;
#pragma unroll
  for (int k = 0; k < 10; ++k) { w[k] = svzero(); cf[k] = mk(0, 0, 0); }
  if (!(P.flags & BEZ_FLAG_NO_SELF_COLLISION)) {
    static_for<BEZ_NCPAIR>([&](auto Q) {
      constexpr int pr = decltype(Q)::value;
      constexpr int ia = BEZ_CPAIR[pr][0], ib = BEZ_CPAIR[pr][1];
      if constexpr (self_part_owns(PART, ia, ib)) {
        constexpr int sa = self_index(BEZ_CAP_LINK[ia]), sb = self_index(BEZ_CAP_LINK[ib]);
        V3 x, f, fn;
        if (self_pair(P, mu, (float)BEZ_CAP_R[ia], (float)BEZ_CAP_R[ib], K.c0[ia], K.c1[ia], K.c0[ib], K.c1[ib], K.V[ia], K.V[ib], x, f, fn)) {
          const SV wr = wrench_at(x, f);
          w[sa] = w[sa] - wr; w[sb] = w[sb] + wr; f2 = fmaf(f.x, f.x, fmaf(f.y, f.y, fmaf(f.z, f.z, f2)));
          const V3 fr = (P.flags & BEZ_FLAG_CF_WITH_FRICTION) ? f : fn;
          cf[sa] = cf[sa] + fr; cf[sb] = cf[sb] - fr;
        }
      }
    });
  }
#pragma unroll
  for (int k = 0; k < 10; ++k) { xs_store_sv(lds, lane, base + k * 9, w[k]); xs_store_v3(lds, lane, base + k * 9 + 6, cf[k]); }
  XS(X_SELFF2 + PART) = f2;   // this part's share of the pairs' sum of |force|^2 (the legs' contact scale)
}
