// The reach table of a collision checker (include/minkhip.h "THE RULE OF THE CERTIFIED SWEEP"): per collision pair and joint, the
// two coefficients that bound how far the joint's motion along an edge can move the pair's geoms against each other.  A model
// constant of a checker, computed from the flat model arrays and the pair list on the host alone — nothing here needs a device, so
// tests/host/motion_bound_cases.cpp walks it under the host sanitizers.  checker_host.hip fills and uploads it on first use.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

namespace mkh {

// MuJoCo's mjtJoint / mjtGeom codes (mkh_types.h and problem_plan.h state them for the kernels and the planner)
enum { MB_JNT_FREE = 0, MB_JNT_BALL = 1, MB_JNT_SLIDE = 2, MB_JNT_HINGE = 3 };
enum { MB_GEOM_PLANE = 0, MB_GEOM_SPHERE = 2, MB_GEOM_CAPSULE = 3, MB_GEOM_ELLIPSOID = 4, MB_GEOM_CYLINDER = 5, MB_GEOM_BOX = 6,
       MB_GEOM_MESH = 7 };

// What the table reads of a model: MkhFlatModel's fields under their names (jnt_qpos0: qpos0 at the joint's first qpos address).
// The mesh arrays may be null in a model without mesh geoms.
struct MotionModel {
  int nbody, njnt;
  const int32_t *body_parentid, *body_jntnum, *body_jntadr;
  const double* body_pos;          // (nbody, 3)
  const int32_t *jnt_type, *jnt_limited;
  const double *jnt_pos /*(njnt, 3)*/, *jnt_range /*(njnt, 2)*/, *jnt_qpos0 /*(njnt,)*/;
  const int32_t *geom_bodyid, *geom_type;
  const double *geom_size /*(ngeom, 3)*/, *geom_pos /*(ngeom, 3)*/;
  const int32_t *geom_dataid, *mesh_vertadr, *mesh_vertnum;
  const double* mesh_vert;         // (nmeshvert, 3), geom frame
};

inline double mb_norm3(const double* v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }

// r_g: the radius of geom g about its own centre (a plane: +inf).
inline double mb_geom_radius(const MotionModel& m, int g) {
  const double* s = m.geom_size + 3 * (size_t)g;
  switch (m.geom_type[g]) {
    case MB_GEOM_SPHERE: return s[0];
    case MB_GEOM_CAPSULE: return s[0] + s[1];
    case MB_GEOM_ELLIPSOID: return std::fmax(s[0], std::fmax(s[1], s[2]));
    case MB_GEOM_CYLINDER: return std::hypot(s[0], s[1]);
    case MB_GEOM_BOX: return mb_norm3(s);
    case MB_GEOM_MESH: {
      const int k = m.geom_dataid ? m.geom_dataid[g] : -1;
      if (k < 0 || !m.mesh_vert) return std::numeric_limits<double>::infinity();       // (no hull to bound: nothing is certified)
      double r = 0.0;
      for (int v = 0; v < m.mesh_vertnum[k]; ++v) r = std::fmax(r, mb_norm3(m.mesh_vert + 3 * ((size_t)m.mesh_vertadr[k] + v)));
      return r;
    }
    default: return std::numeric_limits<double>::infinity();                            // (a plane)
  }
}

// What joint j of its body adds to D: how far it moves the body's origin at most.
inline double mb_joint_shift(const MotionModel& m, int j) {
  const int jt = m.jnt_type[j];
  if (jt == MB_JNT_SLIDE) {
    if (!m.jnt_limited[j]) return std::numeric_limits<double>::infinity();
    return std::fmax(std::fabs(m.jnt_range[2 * j] - m.jnt_qpos0[j]), std::fabs(m.jnt_range[2 * j + 1] - m.jnt_qpos0[j]));
  }
  if (jt == MB_JNT_HINGE || jt == MB_JNT_BALL) return 2.0 * mb_norm3(m.jnt_pos + 3 * (size_t)j);
  return std::numeric_limits<double>::infinity();                                       // (a free joint)
}

// D_after(c, j): the joints of body c behind joint j; j = the body's first joint − 1: D(c).
inline double mb_body_shift(const MotionModel& m, int c, int after) {
  double d = 0.0;
  if (m.body_jntnum[c] < 1) return d;
  for (int j = m.body_jntadr[c]; j < m.body_jntadr[c] + m.body_jntnum[c]; ++j)
    if (j > after) d += mb_joint_shift(m, j);
  return d;
}

// The bodies from the world's child down to b.
inline std::vector<int> mb_chain(const MotionModel& m, int b) {
  std::vector<int> up;
  for (int x = b; x > 0; x = m.body_parentid[x]) up.push_back(x);
  return std::vector<int>(up.rbegin(), up.rend());
}

// out: (n_pairs, njnt, 2) doubles — [k][j][0] multiplies joint j's linear weight of an edge, [k][j][1] its angular weight.
inline void motion_reach(const MotionModel& m, int n_pairs, const int32_t* geom_pairs, double* out) {
  for (size_t i = 0; i < (size_t)n_pairs * m.njnt * 2; ++i) out[i] = 0.0;
  for (int k = 0; k < n_pairs; ++k) {
    const int g[2] = {geom_pairs[2 * k], geom_pairs[2 * k + 1]};
    const std::vector<int> ch[2] = {mb_chain(m, m.geom_bodyid[g[0]]), mb_chain(m, m.geom_bodyid[g[1]])};
    size_t common = 0;                                         // (joints on common ancestors move both geoms rigidly together)
    while (common < ch[0].size() && common < ch[1].size() && ch[0][common] == ch[1][common]) ++common;
    for (int side = 0; side < 2; ++side) {
      // below: what lies between the origin of the body whose joints are being judged and the far side of the geom
      double below = mb_norm3(m.geom_pos + 3 * (size_t)g[side]) + mb_geom_radius(m, g[side]);
      for (size_t t = ch[side].size(); t-- > common;) {
        const int c = ch[side][t];
        if (m.body_jntnum[c] > 0)
          for (int j = m.body_jntadr[c]; j < m.body_jntadr[c] + m.body_jntnum[c]; ++j) {
            double* const o = out + ((size_t)k * m.njnt + j) * 2;
            const int jt = m.jnt_type[j];
            o[0] = (jt == MB_JNT_SLIDE || jt == MB_JNT_FREE) ? 1.0 : 0.0;
            o[1] = jt == MB_JNT_SLIDE ? 0.0 : mb_norm3(m.jnt_pos + 3 * (size_t)j) + mb_body_shift(m, c, j) + below;
          }
        below += mb_norm3(m.body_pos + 3 * (size_t)c) + mb_body_shift(m, c, m.body_jntadr[c] - 1);
      }
    }
  }
}

}  // namespace mkh
