// The clearance of ONE row of q on the LPR lanes of its group (include/minkhip.h "THE RULE OF CLEARANCE"): the body of
// clearance_kernel (clearance.hip: rows of q in memory) and of sweep_kernel (sweep.hip: rows of q blended in LDS between the two
// ends of an edge), so that a swept sample is the clearance of its row, bit for bit.  The body poses go into the group's LDS
// slice level by level (mj_kinematics: the arithmetic of wide_kernel.h's FK and of convex_pre.hip's cv_chain_pose); the group's
// lanes then stride over the checker's pairs — bounding spheres first where the checker has cull records, the analytic routines
// of collide_dev.h behind them; the minimum over the pairs is an exact reduction of order-preserving integer keys (no rounding,
// ties to the lowest pair index).  No atomics, no scratch.
#pragma once
#include <hip/hip_runtime.h>

#include "mkh_types.h"
#include "wave_ops.h"
#include "collide_dev.h"
#include "wide_types.h"

namespace mkh {

// IEEE order of x as unsigned integer order, NaN below everything (a NaN term decides the row: in collision, never free)
__device__ __forceinline__ unsigned long long clr_key(double x) {
  if (x != x) return 0ull;
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ V3 clr_sel(bool s, V3 a, V3 b) { return {s ? a.x : b.x, s ? a.y : b.y, s ? a.z : b.z}; }
__device__ __forceinline__ Q4 clr_sel(bool s, Q4 a, Q4 b) { return {s ? a.w : b.w, s ? a.x : b.x, s ? a.y : b.y, s ? a.z : b.z}; }

// The distance of collide_dev.h's box_box_local (geom_distance's box–box branch) without its witness points, the columns of R
// picked by selects: the routine there indexes the matrix with a loop counter, which puts it into scratch in every kernel that
// compiles it in — and this kernel has none.  Same tests, same order, same arithmetic.
__device__ __forceinline__ double clr_box_box(V3 sa, V3 p1, Q4 q1, V3 sb, V3 p2, Q4 q2, double margin) {
  const M3 R1 = qmat(q1), R2 = qmat(q2);
  M3 R;                                                       // A's axes in B's frame: R2ᵀ·R1
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      R.m[3 * i + j] = R2.m[i] * R1.m[j] + R2.m[3 + i] * R1.m[3 + j] + R2.m[6 + i] * R1.m[6 + j];
  const V3 c = mulT(R2, p1 - p2);
  const V3 c0{R.m[0], R.m[3], R.m[6]}, c1{R.m[1], R.m[4], R.m[7]}, c2{R.m[2], R.m[5], R.m[8]};
  auto column = [&](int i) {
    return V3{i == 0 ? c0.x : (i == 1 ? c1.x : c2.x), i == 0 ? c0.y : (i == 1 ? c1.y : c2.y), i == 0 ? c0.z : (i == 1 ? c1.z : c2.z)};
  };
  double best_sep = -1e300;
#pragma unroll 1
  for (int i = 0; i < 15; ++i) {
    V3 L;
    if (i < 3) L = unit(i);
    else if (i < 6) L = column(i - 3);
    else {
      L = cross(column((i - 6) / 3), unit((i - 6) % 3));
      const double n2 = dot(L, L);
      if (n2 < 1e-18) continue;
      L = (1.0 / sqrt(n2)) * L;
    }
    const double ra = dot(vabs(mulT(R, L)), sa), rb = dot(vabs(L), sb), cl = dot(c, L);
    const double sep = fabs(cl) - (ra + rb);
    if (sep > best_sep) best_sep = sep;
  }
  if (best_sep <= 0.0) return best_sep > margin ? margin : best_sep;
  double best = 1e300;
#pragma unroll 1
  for (int i = 0; i < 8; ++i) {
    const V3 sg{(i & 1) ? 1.0 : -1.0, (i & 2) ? 1.0 : -1.0, (i & 4) ? 1.0 : -1.0};
    const V3 va = c + mul(R, vmulc(sg, sa));
    V3 cl = vclamp(va, sb);
    double d2 = dot(va - cl, va - cl);
    if (d2 < best) best = d2;
    const V3 ul = mulT(R, vmulc(sg, sb) - c);
    cl = vclamp(ul, sa);
    d2 = dot(ul - cl, ul - cl);
    if (d2 < best) best = d2;
  }
#pragma unroll 1
  for (int ea = 0; ea < 12; ++ea) {
    V3 a0, a1;
    box_edge(sa, ea, a0, a1);
    const V3 e1 = c + mul(R, a0), d1 = mul(R, a1 - a0);
    const double a = dot(d1, d1);
#pragma unroll 1
    for (int eb = 0; eb < 12; ++eb) {
      V3 e2, f2;
      box_edge(sb, eb, e2, f2);
      const V3 d2v = f2 - e2, r = e1 - e2;
      const double e = dot(d2v, d2v), f = dot(d2v, r), cc = dot(d1, r), b = dot(d1, d2v);
      const double den = a * e - b * b;
      double sp = (den > 1e-15 * a * e) ? clampd((b * f - cc * e) / den, 0.0, 1.0) : 0.0;
      double t = (b * sp + f) / e;
      if (t < 0.0) { t = 0.0; sp = clampd(-cc / a, 0.0, 1.0); }
      else if (t > 1.0) { t = 1.0; sp = clampd((b - cc) / a, 0.0, 1.0); }
      const V3 x1 = e1 + sp * d1, x2 = e2 + t * d2v;
      const double dd = dot(x1 - x2, x1 - x2);
      if (dd < best) best = dd;
    }
  }
  const double dist = sqrt(best);
  return dist > margin ? margin : dist;
}

// Minimum over the LPR lanes of a row of the wavefront (LPR = 16: one DPP row; 64: the wavefront), in every lane of the row.
template <int LPR>
__device__ __forceinline__ unsigned clr_min_u32(unsigned x) {
  x = umin32(x, dpp_u32<0xB1>(x));
  x = umin32(x, dpp_u32<0x4E>(x));
  x = umin32(x, dpp_u32<0x141>(x));
  x = umin32(x, dpp_u32<0x140>(x));                          // every lane of a 16-lane row now holds the row's minimum
  if constexpr (LPR == 64) {
    const unsigned a = (unsigned)__builtin_amdgcn_readlane((int)x, 0), b = (unsigned)__builtin_amdgcn_readlane((int)x, 16);
    const unsigned c = (unsigned)__builtin_amdgcn_readlane((int)x, 32), d = (unsigned)__builtin_amdgcn_readlane((int)x, 48);
    x = umin32(umin32(a, b), umin32(c, d));
  }
  return x;
}

struct ClrRow {                    // in every lane of the group
  double margin;
  int pair, n_violated;
};

// sX: the group's 7·nbody doubles of LDS (one array per component: x y z | w x y z).  sq: the row of q (nq,) — memory or LDS.
// bad_q: the row has a NaN or an infinite entry (every d_k is NaN: the rule states it; the distance routines' clamps and range
// tests would swallow a NaN, and a capsule–capsule pair would come out at its cap).  cv / cv_row: the (·, n_cv, 7) records of
// convex_contacts_kernel and the row's index there (read only for pairs with a cv_slot).  distance_row: (n_pairs,) or null.
// CVS: the doubles of one record there — the 7 of convex_contacts_kernel, or 1 where convex_sweep_kernel left the distance alone.
// Every lane of the wavefront calls it (wave_sync inside): a group without a row of its own repeats another's.
template <int LPR, int CVS = 7>
__device__ __forceinline__ ClrRow clr_row(const WideProblem& P, double* const sX, const double* const sq, bool bad_q, int sub, int grp,
                                          int n_cv, const double* __restrict__ cv, size_t cv_row, double* __restrict__ distance_row) {
  const int nbody = P.nbody, XS = nbody, n_pairs = P.n_pairs;
  // ---- FK, level by level (mj_kinematics)
  for (int lv = 0; lv < P.nlevels; ++lv) {
    for (int idx = P.level_start[lv] + sub; idx < P.level_start[lv + 1]; idx += LPR) {
      const int b = P.level_body[idx];
      V3 xp{0, 0, 0};
      Q4 xq{1, 0, 0, 0};
      if (b > 0) {
        const int pa = P.body_parent[b];
        const Q4 pq{sX[3 * XS + pa], sX[4 * XS + pa], sX[5 * XS + pa], sX[6 * XS + pa]};
        xp = V3{sX[pa], sX[XS + pa], sX[2 * XS + pa]} + qrot(pq, V3{P.body_pos[3 * b], P.body_pos[3 * b + 1], P.body_pos[3 * b + 2]});
        xq = qmul(pq, Q4{P.body_quat[4 * b], P.body_quat[4 * b + 1], P.body_quat[4 * b + 2], P.body_quat[4 * b + 3]});
        const int jadr = P.body_jntadr[b], jnum = P.body_jntnum[b];
        for (int jn = 0; jn < jnum; ++jn) {
          const int j = jadr + jn, jt = P.jnt_type[j], qa = P.jnt_qadr[j];
          const V3 axl{P.jnt_axis[3 * j], P.jnt_axis[3 * j + 1], P.jnt_axis[3 * j + 2]};
          const V3 jp{P.jnt_pos[3 * j], P.jnt_pos[3 * j + 1], P.jnt_pos[3 * j + 2]};
          if (jt == JNT_FREE) {
            xp = {sq[qa], sq[qa + 1], sq[qa + 2]};
            xq = qnormalize(Q4{sq[qa + 3], sq[qa + 4], sq[qa + 5], sq[qa + 6]});
          }
          const V3 ax = qrot(xq, axl), an = xp + qrot(xq, jp);
          if (jt == JNT_SLIDE) {
            xp = xp + (sq[qa] - P.jnt_qpos0[j]) * ax;
          } else if (jt == JNT_HINGE || jt == JNT_BALL) {
            const Q4 qloc = (jt == JNT_HINGE) ? axis_angle(axl, sq[qa] - P.jnt_qpos0[j])
                                              : qnormalize(Q4{sq[qa], sq[qa + 1], sq[qa + 2], sq[qa + 3]});
            xq = qmul(xq, qloc);
            xp = an - qrot(xq, jp);
          }
        }
        xq = qnormalize(xq);
      }
      sX[b] = xp.x; sX[XS + b] = xp.y; sX[2 * XS + b] = xp.z;
      sX[3 * XS + b] = xq.w; sX[4 * XS + b] = xq.x; sX[5 * XS + b] = xq.y; sX[6 * XS + b] = xq.z;
    }
    wave_sync();
  }
  // ---- the pairs: lane l of the group takes pairs l, l + LPR, …  (ascending, so a strict < keeps the lowest index of a lane's ties)
  unsigned long long best_key = ~0ull;
  double best_m = __builtin_huge_val();
  int best_k = 0x7fffffff, nviol = 0;
  const PairCull* const cull = P.cull;
  for (int k0 = 0; k0 < n_pairs; k0 += LPR) {
    const int k = k0 + sub;
    bool viol = false;
    if (k < n_pairs) {
      const CollisionPairDev& cp = P.pairs[k];
      const int b1 = cp.body1, b2 = cp.body2;
      const Q4 bq1{sX[3 * XS + b1], sX[4 * XS + b1], sX[5 * XS + b1], sX[6 * XS + b1]}, bq2{sX[3 * XS + b2], sX[4 * XS + b2], sX[5 * XS + b2], sX[6 * XS + b2]};
      const V3 bp1{sX[b1], sX[XS + b1], sX[2 * XS + b1]}, bp2{sX[b2], sX[XS + b2], sX[2 * XS + b2]};
      double dist = cp.ddetect;                                // (a pair the cull skips: what mj_geomDistance says about it)
      bool near = true;
      if (cull) {
        const PairCull& c = cull[k];
        const V3 d = (bp2 + qrot(bq2, V3{c.lpos2[0], c.lpos2[1], c.lpos2[2]})) - (bp1 + qrot(bq1, V3{c.lpos1[0], c.lpos1[1], c.lpos1[2]}));
        near = !(dot(d, d) > c.reach2);
      }
      if (bad_q) {
        dist = __builtin_nan("");
      } else if (near) {
        if (cp.cv_slot >= 0) {
          dist = cv[(cv_row * n_cv + cp.cv_slot) * CVS];
        } else {
          const V3 gp1 = bp1 + qrot(bq1, V3{cp.lpos1[0], cp.lpos1[1], cp.lpos1[2]});
          const V3 gp2 = bp2 + qrot(bq2, V3{cp.lpos2[0], cp.lpos2[1], cp.lpos2[2]});
          const Q4 gq1 = qmul(bq1, Q4{cp.lquat1[0], cp.lquat1[1], cp.lquat1[2], cp.lquat1[3]});
          const Q4 gq2 = qmul(bq2, Q4{cp.lquat2[0], cp.lquat2[1], cp.lquat2[2], cp.lquat2[3]});
          const V3 sz1{cp.size1[0], cp.size1[1], cp.size1[2]}, sz2{cp.size2[0], cp.size2[1], cp.size2[2]};
          const int t1 = cp.type1, t2 = cp.type2;
          // geom_distance sorts a pair by type code; sorted here, it has nothing to swap, and behind the test for a box in front
          // (box–box: the twin above) its own box–box routine is dead code, and the 72 bytes of scratch of its indexed matrix with it
          const bool flip = t1 > t2;
          const int ta = flip ? t2 : t1, tb = flip ? t1 : t2;
          if (ta == GEOM_BOX) {
            dist = clr_box_box(sz1, gp1, gq1, sz2, gp2, gq2, cp.ddetect);
          } else {
            __builtin_assume(ta <= tb);
            V3 from, to;
            geom_distance<false, false>(ta, clr_sel(flip, sz2, sz1), clr_sel(flip, gp2, gp1), clr_sel(flip, gq2, gq1), tb, clr_sel(flip, sz1, sz2),
                                        clr_sel(flip, gp1, gp2), clr_sel(flip, gq1, gq2), cp.ddetect, dist, from, to);
          }
        }
      }
      if (distance_row) distance_row[k] = dist;
      viol = !(dist >= cp.dmin);
      const double m = (dist - cp.dmin) + 0.0;                  // (+ 0.0: −0 and +0 are one value to the minimum)
      const unsigned long long key = clr_key(m);
      if (key < best_key) { best_key = key; best_m = m; best_k = k; }
    }
    const unsigned long long vb = __ballot(viol);
    nviol += (int)__builtin_popcountll(LPR == 64 ? vb : (vb >> (grp * LPR)) & ((1ull << (LPR & 63)) - 1ull));
  }
  // ---- the minimum over the group's lanes, exactly: high words, then low words among their ties, then the pair index among those
  const unsigned kh = (unsigned)(best_key >> 32), kl = (unsigned)best_key;
  const unsigned mh = clr_min_u32<LPR>(kh);
  const unsigned ml = clr_min_u32<LPR>(kh == mh ? kl : 0xffffffffu);
  const bool tie = kh == mh && kl == ml;
  const int kmin = (int)clr_min_u32<LPR>(tie ? (unsigned)best_k : 0xffffffffu);
  const double mmin = bperm_f64(best_m, grp * LPR + (kmin & (LPR - 1)));     // (the lane of the group that holds pair kmin)
  return {mmin, kmin, nviol};
}

}  // namespace mkh
