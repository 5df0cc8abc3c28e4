// bez_ws_quad.inc -- lane-group forms of the leg roles' serial passes (bez_step_ws8q.hip: four lanes per env).  Included INSIDE
// namespace w8q behind bez_ws_common.inc.
//
// A quad's lane 2r + c holds block (r, c) of a 6 x 6 spatial matrix [[A, B], [B^T, C]] in full (nine registers) and the row half r
// (0 = angular, 1 = linear) of every spatial vector of the recursion.  A matrix-vector product is nine multiply-adds per lane and one
// quad_perm [1,0,3,2] add per component (the two column halves), a dot product three multiply-adds and one quad_perm [2,3,0,1] add (the
// two row halves), the column half of U for the rank-1 update comes from the other row pair (quad_perm [2,3,0,1]).  DPP only: no LDS
// round trip, no MFMA hop (tools/lanegroup_probe.py, mapping D: x 1.78 on the recursion against one lane per env; 8 lanes per env
// with ds_swizzle broadcasts x 1.48, the MFMA rank-1 update x 0.97).
// Everything per env that is NOT split (kinematics, link inertias, drive terms, contacts) runs redundantly in the four lanes, whose
// LDS columns stay private -- so the hand-overs between the roles are the production kernel's, except the legs' X_IA blocks, which the
// legs leave in the quad's native layout (slot k < 9: entry k of the lane's block; slots 9..11: the lane's half of the bias) and the
// root role gathers from the owning columns.

BEZ_DEV float qp_flip_c(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1 /* quad_perm [1,0,3,2] */, 0xF, 0xF, true)); }
BEZ_DEV float qp_flip_r(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E /* quad_perm [2,3,0,1] */, 0xF, 0xF, true)); }
BEZ_DEV V3 qp_flip_c(V3 v) { return mk(qp_flip_c(v.x), qp_flip_c(v.y), qp_flip_c(v.z)); }
BEZ_DEV V3 qp_flip_r(V3 v) { return mk(qp_flip_r(v.x), qp_flip_r(v.y), qp_flip_r(v.z)); }

// a lane's place in its quad; ca / cs / cm: the lane's coefficients of (Ibar, skew(h), m 1) in its block of a link inertia
struct Quad { bool r, c, diag; float ca, cs, cm; int lane_r; };
BEZ_DEV Quad quad_of(int lane) {
  Quad Q;
  Q.r = (lane & 2) != 0; Q.c = (lane & 1) != 0; Q.diag = Q.r == Q.c;
  Q.ca = (!Q.r && !Q.c) ? 1.f : 0.f; Q.cs = (!Q.r && Q.c) ? 1.f : ((Q.r && !Q.c) ? -1.f : 0.f); Q.cm = (Q.r && Q.c) ? 1.f : 0.f;
  Q.lane_r = lane + (Q.r ? 3 * WS_LANES : 0);   // as the `lane` of an XS access: the row half of a spatial vector stored in six slots
  return Q;
}
BEZ_DEV V3 q_half(SV v, bool lin) { return mk(lin ? v.l.x : v.a.x, lin ? v.l.y : v.a.y, lin ? v.l.z : v.a.z); }
BEZ_DEV SV q_full(V3 h, const Quad& Q) {   // both halves from the two row pairs
  const V3 o = qp_flip_r(h);
  return mksv(mk(Q.r ? o.x : h.x, Q.r ? o.y : h.y, Q.r ? o.z : h.z), mk(Q.r ? h.x : o.x, Q.r ? h.y : o.y, Q.r ? h.z : o.z));
}
BEZ_DEV float q_dot(V3 a, V3 b) { const float d = dot(a, b); return d + qp_flip_r(d); }   // dot of two spatial vectors held as row halves

struct Blk { float m[9]; };   // row-major 3 x 3
BEZ_DEV Blk blk_of(const Sym6& I, const Quad& Q) {
  const float A[9] = {I.A.xx, I.A.xy, I.A.xz, I.A.xy, I.A.yy, I.A.yz, I.A.xz, I.A.yz, I.A.zz};
  const float C[9] = {I.C.xx, I.C.xy, I.C.xz, I.C.xy, I.C.yy, I.C.yz, I.C.xz, I.C.yz, I.C.zz};
  const float B[9] = {I.B.m00, I.B.m01, I.B.m02, I.B.m10, I.B.m11, I.B.m12, I.B.m20, I.B.m21, I.B.m22};
  Blk M;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) M.m[3 * i + j] = Q.r ? (Q.c ? C[3 * i + j] : B[3 * j + i]) : (Q.c ? B[3 * i + j] : A[3 * i + j]);
  return M;
}
BEZ_DEV void blk_add(Blk& M, const Blk& G) {
#pragma unroll
  for (int k = 0; k < 9; ++k) M.m[k] += G.m[k];
}
// M += the lane's block of a link inertia [[Ibar, skew(h)], [skew(h)^T, m 1]]  (add_link_inertia)
BEZ_DEV void blk_add_link(Blk& M, const LinkInertia& I, const Quad& Q) {
  const float cmm = Q.cm * I.m;
  M.m[0] += fmaf(Q.ca, I.Ibar.xx, cmm); M.m[4] += fmaf(Q.ca, I.Ibar.yy, cmm); M.m[8] += fmaf(Q.ca, I.Ibar.zz, cmm);
  M.m[1] += fmaf(Q.ca, I.Ibar.xy, -Q.cs * I.h.z); M.m[2] += fmaf(Q.ca, I.Ibar.xz, Q.cs * I.h.y);
  M.m[3] += fmaf(Q.ca, I.Ibar.xy, Q.cs * I.h.z);  M.m[5] += fmaf(Q.ca, I.Ibar.yz, -Q.cs * I.h.x);
  M.m[6] += fmaf(Q.ca, I.Ibar.xz, -Q.cs * I.h.y); M.m[7] += fmaf(Q.ca, I.Ibar.yz, Q.cs * I.h.x);
}
// ---- link packages handed over through LDS (default asset, no per-env parameters): the arm role of a side (idle for two thirds of the
// legs' pass 2) walks the leg's three hip links once more after B1 and leaves each link's package -- link inertia about the reference
// point (m, h, Ibar: 10 floats) and bias force (6) -- in the column of the quad's lane k for link k, slots X_PKG + side * 16 ..; the
// leg reads 13 words per joint instead of evaluating the package (~125 instructions that the compiler had sunk into pass 2).  The
// legs' pass 2 runs foot -> hip, so the hip links are needed last: the producer is done long before (a sequence word says so:
// ws_pkg_publish / ws_pkg_wait, lanes 2 / 3 of the X_PAIRSEQ slot).
constexpr int PKG_LINKS = 4;
// ... and the ankle / foot links (needed first, right behind B1) come from the two leg<->leg pair roles, which walk both legs down to
// the feet in the window of pass 1 anyway: role 6 leaves the right leg's, role 7 the left leg's, before B1 -- the barrier orders the
// hand-over.  15 floats per link (the mass is a constant of the default asset) in the free slots 12..26 of the leg's own X_IA block,
// columns 0 / 1 of the quad.  With both hand-overs the leg role evaluates no package at all.
BEZ_DEV constexpr int pkg_col(int i) { return i < PKG_LINKS ? i : i - PKG_LINKS; }
BEZ_DEV void ws_pkg_publish(float* lds, int side, int seq) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  lds_word_t* flag = (lds_word_t*)(lds + X_PAIRSEQ * WS_LANES);
  flag[2 + side] = seq;
}
BEZ_DEV void ws_pkg_wait(const float* lds, int side, int seq) {
  lds_word_t* flag = (lds_word_t*)(lds + X_PAIRSEQ * WS_LANES);
#pragma unroll 1
  for (int guard = 0; guard < (1 << 16) && flag[2 + side] < seq; ++guard) __builtin_amdgcn_s_sleep(1);
  if (flag[2 + side] < seq) ws_spin_timeout(lds);   // still missing after the bound (bez_ws_common.inc)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}
template <int L>
BEZ_DEV void wq_store_package(float* lds, int lane, int side, int i, V3 g, const M3& E, V3 r, SV V) {   // i >= PKG_LINKS: the pair roles' hand-over
  LinkInertia LI; SV pl;
  link_inertia<L, false>(1.f, g, E, r, V, LI, pl);
  float* col = lds + (lane & ~3) + (i - PKG_LINKS);
  const float v[16] = {LI.m, LI.h.x, LI.h.y, LI.h.z, LI.Ibar.xx, LI.Ibar.yy, LI.Ibar.zz, LI.Ibar.xy, LI.Ibar.xz, LI.Ibar.yz,
                       pl.a.x, pl.a.y, pl.a.z, pl.l.x, pl.l.y, pl.l.z};
#pragma unroll
  for (int k = 1; k < 16; ++k) col[(X_IA + side * 27 + 12 - 1 + k) * WS_LANES] = v[k];
}
template <int LEG_FIRST>
BEZ_DEV void wq_produce_packages(const Params& P, V3 g, float* lds, int lane, int side, int seq) {
  const M3 E0 = quat_to_mat(XS(X_ROOT + 3), XS(X_ROOT + 4), XS(X_ROOT + 5), XS(X_ROOT + 6));
  M3 E = E0; V3 r = mk(0, 0, 0);
  SV V = mksv(xs_load_v3(lds, lane, X_ROOT + 10), xs_load_v3(lds, lane, X_ROOT + 7)), Sj, cbj;
  float* col = lds + (lane & ~3);
  static_for<PKG_LINKS>([&](auto I) {
    constexpr int i = decltype(I)::value;
    link_kinematics<LEG_FIRST + i>(XS(X_LEGQ + side * 12 + i), XS(X_LEGQ + side * 12 + 6 + i), E, r, V, Sj, cbj);
    LinkInertia LI; SV pl;
    link_inertia<LEG_FIRST + i, false>(1.f, g, E, r, V, LI, pl);
    const float v[16] = {LI.m, LI.h.x, LI.h.y, LI.h.z, LI.Ibar.xx, LI.Ibar.yy, LI.Ibar.zz, LI.Ibar.xy, LI.Ibar.xz, LI.Ibar.yz,
                         pl.a.x, pl.a.y, pl.a.z, pl.l.x, pl.l.y, pl.l.z};
#pragma unroll
    for (int k = 0; k < 16; ++k) col[(X_PKG + side * 16 + k) * WS_LANES + i] = v[k];   // (the quad's four lanes store the same word)
  });
  ws_pkg_publish(lds, side, seq);
}
// M += the lane's block of link I's inertia, pA += the lane's half of its bias force, from the package in LDS
// (pkg / pkg_r: the quad's column-0 address of slot X_PKG, plain and shifted to the lane's half of the bias force -- every package word is
// then within the 16-bit immediate offset of an LDS read; formed per access the compiler hoisted 13 addresses per link out of the substep
// loop and spilled them)
struct PkgBase { const float* a; const float* r; };
BEZ_DEV PkgBase pkg_base(const float* lds, int lane, const Quad& Q) {
  PkgBase B;
  B.a = lds + X_PKG * WS_LANES + (lane & ~3);
  B.r = B.a + (Q.r ? 3 * WS_LANES : 0);
  asm volatile("" : "+v"(B.a), "+v"(B.r));
  return B;
}
template <int I, int LINK>
BEZ_DEV void blk_add_link_pkg(Blk& M, V3& pA, const PkgBase& B, int side, const Quad& Q) {
  constexpr int col = pkg_col(I);
  const int s0 = (I < PKG_LINKS ? side * 16 : X_IA + side * 27 + 12 - 1 - X_PKG);   // relative to X_PKG
  auto at = [&](int k) { return B.a[(s0 + k) * WS_LANES + col]; };
  LinkInertia L;
  L.m = I < PKG_LINKS ? at(0) : (float)link_mass<false>(LINK); L.h = mk(at(1), at(2), at(3));
  L.Ibar.xx = at(4); L.Ibar.yy = at(5); L.Ibar.zz = at(6); L.Ibar.xy = at(7); L.Ibar.xz = at(8); L.Ibar.yz = at(9);
  const V3 pl = mk(B.r[(s0 + 10) * WS_LANES + col], B.r[(s0 + 11) * WS_LANES + col], B.r[(s0 + 12) * WS_LANES + col]);
  blk_add_link(M, L, Q);
  pA = pA + pl;
}
BEZ_DEV V3 blk_mul(const Blk& M, V3 v) {
  return mk(fmaf(M.m[0], v.x, fmaf(M.m[1], v.y, M.m[2] * v.z)), fmaf(M.m[3], v.x, fmaf(M.m[4], v.y, M.m[5] * v.z)),
            fmaf(M.m[6], v.x, fmaf(M.m[7], v.y, M.m[8] * v.z)));
}
// M += k u v^T
BEZ_DEV void blk_add_outer(Blk& M, V3 u, V3 v, float k) {
  const float kx = k * u.x, ky = k * u.y, kz = k * u.z;
  M.m[0] = fmaf(kx, v.x, M.m[0]); M.m[1] = fmaf(kx, v.y, M.m[1]); M.m[2] = fmaf(kx, v.z, M.m[2]);
  M.m[3] = fmaf(ky, v.x, M.m[3]); M.m[4] = fmaf(ky, v.y, M.m[4]); M.m[5] = fmaf(ky, v.z, M.m[5]);
  M.m[6] = fmaf(kz, v.x, M.m[6]); M.m[7] = fmaf(kz, v.y, M.m[7]); M.m[8] = fmaf(kz, v.z, M.m[8]);
}

// per-joint data a leg keeps between pass 2 and pass 3: the lane's row halves of U/D, S and c, the held-parent acceleration, 1/D
template <bool DF> struct P3q { V3 UD; float uD, Dinv; V3 S, cb; };
template <> struct P3q<true> { V3 UD; float uD, Dinv; V3 S, cb; float c0; };   // (c0, and U in UD of a locked joint: struct P3 of bez_ws_common.inc)

// ---- pass 2 of a leg (ws_chain_pass2 in the quad form).  Out: the lane's block of the chain's articulated inertia and its half of the bias.
template <bool DF, int FIRST, int LEN, bool PKG>
BEZ_DEV void wq_chain_pass2(const Params& P, const Quad& Q, float* lds, int lane, int side, int seq, const float* kps, const float* kds, const float* lo, const float* hi,
                            const float* q, const float* qd, const float* target, const LinkInertia* LI, const SV* pAl, const SV* Sl,
                            const SV* cbl, const Sym6& Kc, SV pc, bool mine, BallSel& sel, P3q<DF>* p3, Blk& Mo, V3& pAo, DfWord<DF>& dfw) {
  Blk M = blk_of(Kc, Q);
  V3 pA = q_half(pc, Q.r);
  const PkgBase PB = pkg_base(lds, lane, Q);
  static_for<LEN>([&](auto I) {
    constexpr int i = LEN - 1 - decltype(I)::value;
    constexpr int L = FIRST + i;
    if constexpr (PKG) {   // the packages come from the arm role of this side (links 0..3) and from the pair roles (4, 5)
      if constexpr (i == PKG_LINKS - 1) {
        ws_pkg_wait(lds, side, seq);
#ifdef BEZ_WS_STAMPS
        if constexpr (FIRST == 5) WS_STAMP(0, 20);   // the wait is over (left leg, last substep): tools/stamp_probe.py "pass2 pkg wait done"
#endif
      }
      blk_add_link_pkg<i, L>(M, pA, PB, side, Q);
    } else {
      blk_add_link(M, LI[i], Q);
      pA = pA + q_half(pAl[i], Q.r);
    }
    if constexpr (link_has_box(L)) {
      if (mine && sel.link == L) {  // (a quad's lanes work on one env: the branch is uniform within it)
        Sym6 T = sym6zero();
        add_point_stiffness(T, sel.x, sel.A);
        blk_add(M, blk_of(T, Q));
        pA = pA - q_half(wrench_at(sel.x, sel.f0p), Q.r);
      }
    }
    const V3 Sr = q_half(Sl[i], Q.r), Sc = q_half(Sl[i], Q.c), cbr = q_half(cbl[i], Q.r), cbc = q_half(cbl[i], Q.c);
    V3 u = blk_mul(M, Sc);
    u = u + qp_flip_c(u);                       // the lane's row half of U = IA S
    float Dinv, uD, qhp;
    DfJoint<DF> df;
    // (U.c stands in front of the other two dot products where the record reads it again, behind them elsewhere: the orders the two
    // builds were tuned with)
    float ucb;
    if constexpr (DF) ucb = q_dot(u, cbr);
    const float Jraw = q_dot(Sr, u), sp = q_dot(Sr, pA);
    if constexpr (!DF) ucb = q_dot(u, cbr);
    joint_scalar<L>(P, kps[i], kds[i], lo[i], hi[i], q[i], qd[i], target[i], Jraw, sp, ucb, Dinv, uD, qhp, df);
    bool locked = false;
    if constexpr (DF) { dfw.w |= df.bits << (4 * i); locked = (df.bits & DF_LOCK) != 0u; }
    p3[i].UD = locked ? u : u * Dinv; p3[i].uD = qhp; p3[i].Dinv = Dinv; p3[i].S = Sr; p3[i].cb = cbr;
    if constexpr (DF) p3[i].c0 = df.c0 + ucb;
    const V3 uo = qp_flip_r(u);
    const V3 uc = mk(Q.diag ? u.x : uo.x, Q.diag ? u.y : uo.y, Q.diag ? u.z : uo.z);   // the column half of U this block needs
    blk_add_outer(M, u, uc, -Dinv);
    V3 t = blk_mul(M, cbc);
    t = t + qp_flip_c(t);
    pA = pA + t + u * uD;
#ifdef BEZ_WS_STAMPS
    if constexpr (FIRST == 5) { pin(pA); WS_STAMP(0, 26 + i); }   // per-joint progress of the left leg (last substep)
#endif   // (a fence per joint as well: measured slower, 24.49 against 23.88 us)
  });
  Mo = M; pAo = pA;
}

// ---- the leg<->leg correction (ws_chain_self_correction in the quad form); pAo: the lane's half of the chain's bias
template <bool DF, int LEN, bool CL>
BEZ_DEV float wq_chain_self_correction(const Params& P, const Quad& Q, float* lds, int lane, int side, int seq, P3q<DF>* p3, V3& pAo, int slot_bias, DfWord<DF> dfw) {
  static_assert(LEN == 6, "legs only");
  V3 w[LEN];
  static_for<LEN>([&](auto I) {
    constexpr int i = decltype(I)::value;
    if constexpr (i >= 1) w[i] = xs_load_v3(lds, Q.lane_r, X_SELF + (side * 5 + i - 1) * 9) + xs_load_v3(lds, Q.lane_r, X_SELF + 90 + (side * 5 + i - 1) * 9);
  });
  static_for<LEN>([&](auto I) {
    constexpr int i = decltype(I)::value;
    if constexpr (i >= 1) pin(w[i]);
  });
  V3 acc = mk(0, 0, 0), wsub = mk(0, 0, 0);
  float am = 0.f, as = 0.f;
  static_for<LEN>([&](auto I) {
    constexpr int i = LEN - 1 - decltype(I)::value;
    if constexpr (i >= 1) { acc = acc + w[i]; wsub = wsub + w[i]; }
    const float tq = q_dot(p3[i].S, wsub);
    as = fmaf(tq * tq, p3[i].Dinv, as); am = fmaf(-tq, p3[i].uD, am);
    const float sd = -q_dot(p3[i].S, acc);
    if constexpr (DF) {
      const bool lk = ((dfw.w >> (4 * i)) & DF_LOCK) != 0u;   // (as ws_chain_self_correction)
      acc = acc + p3[i].UD * (lk ? 0.f : sd);
      p3[i].Dinv = lk ? sd : sd * p3[i].Dinv;
    } else {
      acc = acc + p3[i].UD * sd;
      p3[i].Dinv = sd * p3[i].Dinv;
    }
  });
  XS(X_SELFSUM + side * 2) = am; XS(X_SELFSUM + side * 2 + 1) = as;
  ws_pair_publish(lds, side, seq);
  ws_pair_wait<CL>(lds, side, seq);
  SelfSums Z;
  Z.am = XS(X_SELFSUM) + XS(X_SELFSUM + 2); Z.as = XS(X_SELFSUM + 1) + XS(X_SELFSUM + 3); Z.f2 = XS(X_SELFF2) + XS(X_SELFF2 + 1);
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
  xs_store_v3(lds, lane, slot_bias, pAo);
  return sc;
}

// ---- pass 3 of a leg (ws_chain_pass3 in the quad form, the record's parameters included); returns the chain-end acceleration (both halves)
template <bool DF, int FIRST, int LEN, bool CL>
BEZ_DEV SV wq_chain_pass3(const Params& P, const Quad& Q, const P3q<DF>* p3, float* q, float* qd, bool mine, const BallSel& sel, V3& fl, V3& f_end,
                          float* lds, int lane, bool keep, bool first, float sc, DfWord<DF> dfw, const float* kps, const float* kds, const float* lo,
                          const float* hi, const float* target, int e, int sub, bool active) {
  V3 a = xs_load_v3(lds, Q.lane_r, X_A0);
  static_for<LEN>([&](auto I) {
    constexpr int i = decltype(I)::value;
    constexpr int L = FIRST + i;
    float qdd;
    if constexpr (DF) {
      const uint32_t dfb = (dfw.w >> (4 * i)) & 15u;
      const float dUa = q_dot(p3[i].UD, a);
      qdd = (dfb & DF_LOCK) ? p3[i].uD : p3[i].uD - dUa;
      if (active) df_record(P, e, sub, L - 1, dfb, kps[i], kds[i], lo[i], hi[i], q[i], qd[i], target[i], qdd, p3[i].c0 + dUa);
    } else {
      qdd = p3[i].uD - q_dot(p3[i].UD, a);
    }
    a = a + p3[i].cb + p3[i].S * qdd;
    const float v = fmaf(P.h, qdd, qd[i]);
    qd[i] = v;
    q[i] = fmaf(P.h, v, q[i]);
    if constexpr (link_has_box(L)) {
      V3 f = xs_self_force(lds, lane, self_index(L)) * sc;
      if (mine && sel.link == L) { fl = sel.f0p - mul(sel.A, point_of(q_full(a, Q), sel.x)); f = f + cf_along(P, fl, sel.n); }
      if (keep) {
        if constexpr (i == LEN - 1) f_end = f;
        else ws_cf_acc(lds, lane, link_body<CL>(L), f, P.cf_w, first);
      }
    }
  });
  return q_full(a, Q);
}

// ---- the root role's side: a leg's X_IA block (quad layout) added to the torso's articulated inertia (complete at B1c: the legs store it
// right behind pass 2) and, separately, to its bias (complete at B2: the leg<->leg correction changes only the bias)
BEZ_DEV void wq_add_leg_inertia(const float* lds, int lane, int slot, Sym6& I) {
  const float* col = lds + (lane & ~3);   // column of the quad's lane (0, 0); + 1: (0, 1) = B, + 2: (1, 0), + 3: (1, 1) = C
  auto at = [&](int k, int o) { return col[(slot + k) * WS_LANES + o]; };
  I.A.xx += at(0, 0); I.A.xy += at(1, 0); I.A.xz += at(2, 0); I.A.yy += at(4, 0); I.A.yz += at(5, 0); I.A.zz += at(8, 0);
  I.B.m00 += at(0, 1); I.B.m01 += at(1, 1); I.B.m02 += at(2, 1); I.B.m10 += at(3, 1); I.B.m11 += at(4, 1); I.B.m12 += at(5, 1);
  I.B.m20 += at(6, 1); I.B.m21 += at(7, 1); I.B.m22 += at(8, 1);
  I.C.xx += at(0, 3); I.C.xy += at(1, 3); I.C.xz += at(2, 3); I.C.yy += at(4, 3); I.C.yz += at(5, 3); I.C.zz += at(8, 3);
}
BEZ_DEV void wq_add_leg_bias(const float* lds, int lane, int slot, SV& p) {
  const float* col = lds + (lane & ~3);
  auto at = [&](int k, int o) { return col[(slot + k) * WS_LANES + o]; };
  p.a = p.a + mk(at(9, 0), at(10, 0), at(11, 0));
  p.l = p.l + mk(at(9, 2), at(10, 2), at(11, 2));
}
BEZ_DEV void xs_add_inertia(const float* lds, int lane, int slot, Sym6& I) {   // the inertia part of a block in the one-lane layout
  float* f = (float*)&I;
#pragma unroll
  for (int i = 0; i < 21; ++i) f[i] += XS(slot + i);
}
// solve_spd6 (bez_spatial.h) in two halves: the factorisation needs the inertia only -- the root role runs it while the legs are still busy
// with their leg<->leg correction -- and the two substitutions need the bias
struct Ldl6 { float L[15]; float dinv[6]; };   // strict lower triangle, row-major: (1,0) (2,0) (2,1) (3,0) ...
BEZ_DEV constexpr int ldl_ix(int i, int j) { return i * (i - 1) / 2 + j; }
BEZ_DEV Ldl6 ldl6_factor(const Sym6& I) {
  float L[6][6];
  L[0][0] = I.A.xx; L[1][0] = I.A.xy; L[1][1] = I.A.yy; L[2][0] = I.A.xz; L[2][1] = I.A.yz; L[2][2] = I.A.zz;
  L[3][0] = I.B.m00; L[3][1] = I.B.m10; L[3][2] = I.B.m20;
  L[4][0] = I.B.m01; L[4][1] = I.B.m11; L[4][2] = I.B.m21;
  L[5][0] = I.B.m02; L[5][1] = I.B.m12; L[5][2] = I.B.m22;
  L[3][3] = I.C.xx; L[4][3] = I.C.xy; L[4][4] = I.C.yy; L[5][3] = I.C.xz; L[5][4] = I.C.yz; L[5][5] = I.C.zz;
  float d[6];
  Ldl6 F;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    float dj = L[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) dj = fmaf(-L[j][k] * L[j][k], d[k], dj);
    d[j] = dj;
    const float inv = frcp(dj);
    F.dinv[j] = inv;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      float s = L[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) s = fmaf(-L[i][k] * L[j][k], d[k], s);
      L[i][j] = s * inv;
    }
  }
#pragma unroll
  for (int i = 1; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < i; ++j) F.L[ldl_ix(i, j)] = L[i][j];
  return F;
}
BEZ_DEV SV ldl6_solve(const Ldl6& F, SV b) {
  float x[6] = {b.a.x, b.a.y, b.a.z, b.l.x, b.l.y, b.l.z};
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int k = 0; k < i; ++k) x[i] = fmaf(-F.L[ldl_ix(i, k)], x[k], x[i]);
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) x[i] = x[i] * F.dinv[i];
#pragma unroll
  for (int i = 5; i >= 0; --i) {
#pragma unroll
    for (int k = i + 1; k < 6; ++k) x[i] = fmaf(-F.L[ldl_ix(k, i)], x[k], x[i]);
  }
  return mksv(mk(x[0], x[1], x[2]), mk(x[3], x[4], x[5]));
}
