// Host-only planning of models and problems (problem_plan.h): table arithmetic and validation, no HIP runtime call, no
// environment.  minkhip.hip uploads what this file plans.
#include "problem_plan.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>

namespace mkh {
namespace {

constexpr double kInf = std::numeric_limits<double>::infinity();

// the error text of a refused model / descriptor (mkh_last_error) and its code
struct Fail {
  std::string& err;
  int32_t operator()(int32_t code, const char* fmt, ...) const {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    err = buf;
    return code;
  }
};

}  // namespace

int32_t plan_model(const MkhFlatModel* h, HostModel& m, std::string& err) {
  const Fail fail{err};
  // (more than 64 bodies or dofs: beyond the wavefront kernels — the workgroup-per-problem kernel takes every call, wide_kernel.h)
  const bool big = h->nbody > kWave || h->nv > kWave;
  if (h->nbody > 4096 || h->nv > 1024) return fail(MKH_E_LIMIT, "nbody=%d / nv=%d: at most 4096 bodies and 1024 dofs", h->nbody, h->nv);
  if (h->nv < 1 || h->nbody < 2) return fail(MKH_E_INVALID, "model has no degrees of freedom");
  m.big = big;
  m.nq = h->nq; m.nv = h->nv; m.nbody = h->nbody; m.njnt = h->njnt; m.ngeom = h->ngeom; m.nsite = h->nsite;
  m.body_ipos.assign(h->body_ipos, h->body_ipos + 3 * h->nbody);
  m.body_mass.assign(h->body_mass, h->body_mass + h->nbody);
  m.body_subtreemass.assign(h->body_subtreemass, h->body_subtreemass + h->nbody);
  auto cpi = [](const int32_t* p, int n) { return std::vector<int32_t>(p, p + n); };
  auto cpd = [](const double* p, int n) { return std::vector<double>(p, p + n); };
  m.body_parentid = cpi(h->body_parentid, h->nbody); m.body_rootid = cpi(h->body_rootid, h->nbody);
  m.body_jntnum = cpi(h->body_jntnum, h->nbody); m.body_jntadr = cpi(h->body_jntadr, h->nbody);
  m.body_dofnum = cpi(h->body_dofnum, h->nbody); m.body_dofadr = cpi(h->body_dofadr, h->nbody);
  m.jnt_type = cpi(h->jnt_type, h->njnt); m.jnt_qposadr = cpi(h->jnt_qposadr, h->njnt);
  m.jnt_dofadr = cpi(h->jnt_dofadr, h->njnt); m.jnt_bodyid = cpi(h->jnt_bodyid, h->njnt);
  m.jnt_limited = cpi(h->jnt_limited, h->njnt); m.jnt_range = cpd(h->jnt_range, h->njnt * 2);
  m.jnt_pos = cpd(h->jnt_pos, h->njnt * 3); m.jnt_axis = cpd(h->jnt_axis, h->njnt * 3);
  for (int j = 0; j < h->njnt; ++j) m.jnt_qpos0.push_back(h->qpos0[h->jnt_qposadr[j]]);
  m.dof_bodyid = cpi(h->dof_bodyid, h->nv); m.dof_jntid = cpi(h->dof_jntid, h->nv);
  m.dof_parentid = cpi(h->dof_parentid, h->nv);
  m.site_bodyid = cpi(h->site_bodyid, h->nsite); m.geom_bodyid = cpi(h->geom_bodyid, h->ngeom);
  m.geom_type = cpi(h->geom_type, h->ngeom);
  m.body_pos = cpd(h->body_pos, h->nbody * 3); m.body_quat = cpd(h->body_quat, h->nbody * 4);
  m.site_pos = cpd(h->site_pos, h->nsite * 3); m.site_quat = cpd(h->site_quat, h->nsite * 4);
  m.geom_size = cpd(h->geom_size, h->ngeom * 3); m.geom_pos = cpd(h->geom_pos, h->ngeom * 3);
  m.geom_quat = cpd(h->geom_quat, h->ngeom * 4);
  m.geom_dataid.assign(h->ngeom, -1);
  if (h->nmesh > 0) {
    if (!h->geom_dataid || !h->mesh_vertadr || !h->mesh_vertnum || !h->mesh_vert || h->nmeshvert < 1)
      return fail(MKH_E_INVALID, "nmesh = %d but a mesh array is null", h->nmesh);
    m.geom_dataid = cpi(h->geom_dataid, h->ngeom);
    m.mesh_vertadr = cpi(h->mesh_vertadr, h->nmesh); m.mesh_vertnum = cpi(h->mesh_vertnum, h->nmesh);
    for (int k = 0; k < h->nmesh; ++k)
      if (m.mesh_vertadr[k] < 0 || m.mesh_vertnum[k] < 1 || m.mesh_vertadr[k] + m.mesh_vertnum[k] > h->nmeshvert)
        return fail(MKH_E_INVALID, "mesh %d: vertex range out of bounds", k);
    for (int g = 0; g < h->ngeom; ++g)
      if (m.geom_dataid[g] >= h->nmesh) return fail(MKH_E_INVALID, "geom %d: mesh id out of range", g);
    m.h_mesh_vert.assign(h->mesh_vert, h->mesh_vert + (size_t)h->nmeshvert * 3);
  }

  const int nb = m.nbody, nv = m.nv;
  // ---- the tree by levels, subtree ranges, the subtree of body 1, dof chains
  std::vector<int32_t> depth(nb, 0);
  int maxdepth = 0;
  for (int b = 1; b < nb; ++b) {
    if (m.body_parentid[b] >= b) return fail(MKH_E_INVALID, "body %d has parent id >= its own id", b);
    depth[b] = depth[m.body_parentid[b]] + 1;
    if (depth[b] > maxdepth) maxdepth = depth[b];
  }
  int nrounds = 0;
  while ((1 << nrounds) < maxdepth) ++nrounds;
  if (!big && nrounds > kMaxRounds) return fail(MKH_E_LIMIT, "kinematic tree too deep");
  m.nrounds = nrounds;
  for (int lv = 0; lv <= maxdepth; ++lv) {
    m.level_start.push_back((int32_t)m.level_body.size());
    for (int b = 0; b < nb; ++b) if (depth[b] == lv) m.level_body.push_back(b);
  }
  m.level_start.push_back((int32_t)m.level_body.size());
  m.nlevels = maxdepth + 1;
  m.subtree_last.resize(nb); m.in_robot.resize(nb); m.jntadr0.resize(nb);
  for (int b = nb - 1; b >= 0; --b) {
    m.subtree_last[b] = b;
    for (int c = b + 1; c < nb; ++c)
      if (m.body_parentid[c] == b && m.subtree_last[c] > m.subtree_last[b]) m.subtree_last[b] = m.subtree_last[c];
  }
  for (int b = 0; b < nb; ++b) {
    m.in_robot[b] = (b >= 1 && m.body_rootid[b] == 1) ? 1 : 0;      // subtree of body 1 (ComTask)
    m.jntadr0[b] = m.body_jntadr[b] < 0 ? 0 : m.body_jntadr[b];
  }
  m.chain_words = (nv + 63) / 64;
  m.chain.assign((size_t)nb * m.chain_words, 0ull);
  for (int b = 1; b < nb; ++b) {                     // dofs on the chain world → body (mj_jac's ancestor walk)
    int x = b;
    while (x > 0 && m.body_dofnum[x] == 0) x = m.body_parentid[x];
    if (x == 0) continue;
    for (int i = m.body_dofadr[x] + m.body_dofnum[x] - 1; i >= 0; i = m.dof_parentid[i])
      m.chain[(size_t)b * m.chain_words + (i >> 6)] |= 1ull << (i & 63);
  }
  // ---- dofs
  m.dof_kind.assign(nv, 0); m.dof_k.assign(nv, 0); m.dof_qadr.assign(nv, -1);
  m.dof_lo.assign(nv, -kInf); m.dof_hi.assign(nv, kInf);
  for (int dd = 0; dd < nv; ++dd) {
    const int j = m.dof_jntid[dd], jt = m.jnt_type[j], k = dd - m.jnt_dofadr[j];
    if (jt == JNT_HINGE) { m.dof_kind[dd] = DOF_HINGE; m.dof_qadr[dd] = m.jnt_qposadr[j]; }
    else if (jt == JNT_SLIDE) { m.dof_kind[dd] = DOF_SLIDE; m.dof_qadr[dd] = m.jnt_qposadr[j]; }
    else if (jt == JNT_BALL) { m.dof_kind[dd] = DOF_BALL; m.dof_k[dd] = k; m.dof_qadr[dd] = m.jnt_qposadr[j]; }
    else if (k < 3) { m.dof_kind[dd] = DOF_FREE_LIN; m.dof_k[dd] = k; }
    else { m.dof_kind[dd] = DOF_FREE_ANG; m.dof_k[dd] = k - 3; }
    // (a limited ball joint: the reference's check_limits compares the quaternion's w with the range — first dof lane)
    if (((jt == JNT_HINGE || jt == JNT_SLIDE) || (jt == JNT_BALL && k == 0)) && m.jnt_limited[j]) {
      m.dof_lo[dd] = m.jnt_range[2 * j]; m.dof_hi[dd] = m.jnt_range[2 * j + 1];
    }
  }

  // ---- body tables
  std::vector<double>& body_f = m.body_f;
  std::vector<int32_t>& body_i = m.body_i;
  body_f.assign(BF_COUNT * 64, 0.0);
  body_i.assign(BI_COUNT * 64, 0);
  if (!big) {                                      // (the lane tables of the wavefront kernels: ≤ 64 bodies / dofs)
    for (int b = 0; b < nb; ++b) {
      for (int k = 0; k < 3; ++k) body_f[(BF_POS + k) * 64 + b] = m.body_pos[3 * b + k];
      for (int k = 0; k < 4; ++k) body_f[(BF_QUAT + k) * 64 + b] = m.body_quat[4 * b + k];
      for (int k = 0; k < 3; ++k) body_f[(BF_IPOS + k) * 64 + b] = m.body_ipos[3 * b + k];
      body_f[BF_MASS * 64 + b] = m.body_mass[b];
      body_f[BF_SUBTREEMASS * 64 + b] = m.body_subtreemass[b];
      body_i[BI_PARENT * 64 + b] = m.body_parentid[b];
      body_i[BI_JNTADR * 64 + b] = m.jntadr0[b];
      body_i[BI_JNTNUM * 64 + b] = m.body_jntnum[b];
      body_i[BI_SUBTREE_LAST * 64 + b] = m.subtree_last[b];
      body_i[BI_IN_ROBOT * 64 + b] = m.in_robot[b];
      // pointer-jumping ancestors: anc_0 = parent, anc_{r+1} = anc_r(anc_r)
      int a = m.body_parentid[b];
      for (int r = 0; r < kMaxRounds; ++r) {
        body_i[(BI_ANC0 + r) * 64 + b] = a;
        // advance 2^r more steps
        int steps = 1 << r, x = a;
        for (int k = 0; k < steps && x > 0; ++k) x = m.body_parentid[x];
        a = x;
      }
    }
    for (int b = 0; b < nb; ++b) {
      int lo = 0;
      for (int r = 0; r < 5 && r < kMaxRounds; ++r) lo |= (body_i[(BI_ANC0 + r) * 64 + b] & 63) << (6 * r);
      body_i[BI_ANCPACK0 * 64 + b] = lo;
      body_i[BI_ANCPACK1 * 64 + b] = kMaxRounds > 5 ? (body_i[(BI_ANC0 + 5) * 64 + b] & 63) : 0;
    }
    // the anc recurrence above must satisfy anc_{r+1}(b) = anc_r(anc_r(b)); verify
    for (int b = 0; b < nb; ++b)
      for (int r = 0; r + 1 < kMaxRounds; ++r) {
        int a = body_i[(BI_ANC0 + r) * 64 + b];
        int aa = body_i[(BI_ANC0 + r) * 64 + a];
        if (body_i[(BI_ANC0 + r + 1) * 64 + b] != aa) return fail(MKH_E_INVALID, "internal: ancestor table");
      }
  }
  // ---- joint arrays
  m.jnt_f.assign(m.njnt * JF_COUNT, 0.0);
  m.jnt_i.assign(m.njnt * JI_COUNT, 0);
  for (int j = 0; j < m.njnt; ++j) {
    for (int k = 0; k < 3; ++k) m.jnt_f[j * JF_COUNT + JF_AXIS + k] = m.jnt_axis[3 * j + k];
    for (int k = 0; k < 3; ++k) m.jnt_f[j * JF_COUNT + JF_POS + k] = m.jnt_pos[3 * j + k];
    m.jnt_f[j * JF_COUNT + JF_QPOS0] = m.jnt_qpos0[j];
    m.jnt_i[j * JI_COUNT + JI_TYPE] = m.jnt_type[j];
    m.jnt_i[j * JI_COUNT + JI_QADR] = m.jnt_qposadr[j];
    m.jnt_i[j * JI_COUNT + JI_DADR] = m.jnt_dofadr[j];
    if (m.jnt_type[j] == JNT_FREE && (m.body_jntnum[m.jnt_bodyid[j]] != 1))
      return fail(MKH_E_INVALID, "free joint must be the only joint of its body");
  }
  // ---- dof tables
  m.dof_i.assign(DI_COUNT * 64, 0);
  m.dof_f.assign(DF_COUNT * 64, 0.0);
  for (int d = 0; d < 64; ++d) { m.dof_f[DF_RANGE_LO * 64 + d] = -kInf; m.dof_f[DF_RANGE_HI * 64 + d] = kInf; m.dof_i[DI_QADR * 64 + d] = -1; }
  for (int d = 0; d < (big ? 0 : nv); ++d) {
    const int j = m.dof_jntid[d];
    m.dof_i[DI_JNT * 64 + d] = j;
    m.dof_i[DI_KIND * 64 + d] = m.dof_kind[d];
    m.dof_i[DI_K * 64 + d] = m.dof_k[d];
    m.dof_i[DI_BODY * 64 + d] = m.dof_bodyid[d];
    m.dof_i[DI_QADR * 64 + d] = m.dof_qadr[d];
    m.dof_i[DI_JIDX * 64 + d] = j - m.body_jntadr[m.jnt_bodyid[j]];
    m.dof_f[DF_RANGE_LO * 64 + d] = m.dof_lo[d];
    m.dof_f[DF_RANGE_HI * 64 + d] = m.dof_hi[d];
  }
  return MKH_OK;
}

namespace {

// Descriptor of the row- and lane-per-problem kernels (quad_kernel.h, lane_kernel.h) of a problem that qualifies: nv ≤ 16
// (row kernel; the lane kernel: nv ≤ 8), at most 16 links on the frames' chains, hinge / slide joints only, plain
// FrameTasks (≤ 8) + PostureTasks + box limits.  Returns the size class (4 / 6 / 7 / 8: both kernels, 16: the row
// kernel only), 0 when the problem stays on the wavefront kernel.
int build_lane_problem(const HostModel& m, const DeviceProblem& P, const std::vector<FrameTaskDev>& ft, const std::vector<double>& pcost,
                       const std::vector<double>& clo, const std::vector<double>& chi, const std::vector<double>& vlim,
                       bool has_relative, LaneProblem2& L) {
  const double inf = kInf;
  if (m.nv > kLaneDescDofs2) return 0;
  if (P.n_frame < 1 || P.n_frame > kLaneMaxFrames || P.n_com > 1 || P.n_pairs || P.n_dense_rows ||
      P.n_dense_limit_rows || P.dense_box)       // (dense_box: per-instance box rows of a plugin limit, wavefront kernels only)
    return 0;
  const bool com = P.n_com == 1;                 // ComTask: the two-row build of the row kernel, every body of the robot a link
  if (com && (m.big || m.body_mass.empty())) return 0;
  // hinge / slide joints; the two-row build of the row kernel (17 … 32 dofs or links) also takes free joints — a floating base
  bool has_free = false;
  for (int j = 0; j < m.njnt; ++j) {
    if (m.jnt_type[j] == JNT_FREE && m.body_jntnum[m.jnt_bodyid[j]] == 1) { has_free = true; continue; }
    if (m.jnt_type[j] != JNT_HINGE && m.jnt_type[j] != JNT_SLIDE) return 0;
  }
  if (m.nq != m.nv + (has_free ? 1 : 0)) return 0;      // (one free joint at most: its quaternion is the extra coordinate)
  memset(&L, 0, sizeof L);
  L.nq = m.nq; L.nv = m.nv; L.n_frame = P.n_frame; L.n_posture = P.n_posture; L.n_cfg = P.n_cfg; L.n_vel = P.n_vel;
  // links = the bodies on the chains world → frame bodies, in body-id order (parents first)
  std::vector<int> need(m.nbody, 0), link_of(m.nbody, -1);
  for (int t = 0; t < P.n_frame; ++t) {
    for (int b = ft[t].body; b > 0; b = m.body_parentid[b]) need[b] = 1;
    if (ft[t].relative)                              // RelativeFrameTask: the root frame's chain as well (two-row build)
      for (int b = ft[t].root_body; b > 0; b = m.body_parentid[b]) need[b] = 1;
  }
  std::vector<char> in_robot(m.nbody, 0);           // subtree of body 1 (mj_jacSubtreeCom(m, d, jac, 1): com_task.py:71-97)
  if (com)
    for (int b = 1; b < m.nbody; ++b) {
      in_robot[b] = b == 1 || in_robot[m.body_parentid[b]];
      if (in_robot[b]) need[b] = 1;
    }
  int nl = 0;
  int free_link[4] = {-1, -1, -1, -1};
  std::vector<int> link_of_jnt(m.njnt, -1);
  // Pose of a jointless body relative to its nearest ancestor that is a link (or the world): folded into the local
  // transforms of its children and of the frames attached to it, so that it costs neither a link nor LDS.
  struct Xf { double p[3], q[4]; };
  auto compose = [](const Xf& a, const double* p, const double* q) {     // a ∘ (p, q)
    Xf r;
    const double w = a.q[0], x = a.q[1], y = a.q[2], z = a.q[3];
    const double tx = 2 * (y * p[2] - z * p[1]), ty = 2 * (z * p[0] - x * p[2]), tz = 2 * (x * p[1] - y * p[0]);
    r.p[0] = a.p[0] + p[0] + w * tx + (y * tz - z * ty);
    r.p[1] = a.p[1] + p[1] + w * ty + (z * tx - x * tz);
    r.p[2] = a.p[2] + p[2] + w * tz + (x * ty - y * tx);
    r.q[0] = w * q[0] - x * q[1] - y * q[2] - z * q[3];
    r.q[1] = w * q[1] + x * q[0] + y * q[3] - z * q[2];
    r.q[2] = w * q[2] - x * q[3] + y * q[0] + z * q[1];
    r.q[3] = w * q[3] + x * q[2] - y * q[1] + z * q[0];
    return r;
  };
  const Xf ident{{0, 0, 0}, {1, 0, 0, 0}};
  std::vector<Xf> fold(m.nbody, ident);
  std::vector<char> folded(m.nbody, 0);
  folded[0] = 1;                                      // the world: identity, link −1
  for (int b = 1; b < m.nbody; ++b) {
    if (!need[b]) continue;
    const int pb = m.body_parentid[b];
    const Xf local = folded[pb] ? compose(fold[pb], &m.body_pos[3 * b], &m.body_quat[4 * b])
                                : compose(ident, &m.body_pos[3 * b], &m.body_quat[4 * b]);
    if (m.body_jntnum[b] == 0) {                     // jointless: fold
      fold[b] = local; folded[b] = 1; link_of[b] = link_of[pb];
      continue;
    }
    // A body with k > 1 joints becomes a chain of k links with identity offsets: mj_kinematics applies a body's
    // joints one after the other in the moving body frame, which is exactly a serial chain of coincident frames.
    if (m.jnt_type[m.body_jntadr[b]] == JNT_FREE) {
      // mj_kinematics: a free body's pose IS its qpos (body_pos / body_quat are not used): three slide links along the world
      // axes from the origin, then the rotation
      const int jj = m.body_jntadr[b];
      if (nl + 4 > kLaneMaxLinks2) return 0;
      for (int i = 0; i < 4; ++i) {
        LaneLink& k = L.link[nl];
        k.parent = i == 0 ? -1 : nl - 1;
        k.quat[0] = 1.0;
        k.jtype = i < 3 ? JNT_SLIDE : JNT_BALL;
        k.dof = m.jnt_dofadr[jj] + (i < 3 ? i : 3);
        k.qadr = m.jnt_qposadr[jj] + 3;
        if (i < 3) k.axis[i] = 1.0;
        free_link[i] = nl++;
      }
      link_of_jnt[jj] = nl - 1;
      link_of[b] = nl - 1;
      continue;
    }
    for (int i = 0; i < m.body_jntnum[b]; ++i) {
      if (nl >= kLaneMaxLinks2) return 0;
      LaneLink& k = L.link[nl];
      k.parent = i == 0 ? link_of[pb] : nl - 1;
      k.quat[0] = 1.0;
      if (i == 0) {
        for (int c = 0; c < 3; ++c) k.pos[c] = local.p[c];
        for (int c = 0; c < 4; ++c) k.quat[c] = local.q[c];
      }
      const int jj = m.body_jntadr[b] + i;
      k.jtype = m.jnt_type[jj]; k.dof = m.jnt_dofadr[jj]; k.qpos0 = m.jnt_qpos0[jj];
      for (int c = 0; c < 3; ++c) { k.axis[c] = m.jnt_axis[3 * jj + c]; k.jpos[c] = m.jnt_pos[3 * jj + c]; }
      link_of_jnt[jj] = nl;
      link_of[b] = nl++;
    }
  }
  L.nlink = nl;
  for (int dd = 0; dd < kLaneDescDofs2; ++dd) { L.dof_link[dd] = -1; L.dof_qadr[dd] = 0; L.range_lo[dd] = -inf; L.range_hi[dd] = inf; }
  for (int dd = 0; dd < m.nv; ++dd) {
    const int j = m.dof_jntid[dd];
    if (m.jnt_type[j] == JNT_FREE) {
      // dofs 0-2: translations along the world axes (the slide links); 3-5: rotations about the body's own axes through its origin
      const int k = dd - m.jnt_dofadr[j];
      L.dof_link[dd] = link_of_jnt[j] < 0 ? -1 : (k < 3 ? free_link[k] : free_link[3]);
      L.dof_qadr[dd] = m.jnt_qposadr[j] + (k < 3 ? k : k + 1);      // (rotations: any finite entry — their posture cost is zero, mink/tasks/posture_task.py:95-99)
      L.dof_axis[dd][k % 3] = 1.0;
      L.dof_slide[dd] = k < 3;
      continue;
    }
    L.dof_link[dd] = link_of_jnt[j];
    L.dof_qadr[dd] = m.jnt_qposadr[j];
    for (int c = 0; c < 3; ++c) { L.dof_axis[dd][c] = m.jnt_axis[3 * j + c]; L.dof_jpos[dd][c] = m.jnt_pos[3 * j + c]; }
    L.dof_slide[dd] = m.jnt_type[j] == JNT_SLIDE;
    if (m.jnt_limited[j]) { L.range_lo[dd] = m.jnt_range[2 * j]; L.range_hi[dd] = m.jnt_range[2 * j + 1]; }
  }
  if (com) {
    L.n_com = 1;
    L.com_rowmask = P.com_rowmask[0];
    for (int k = 0; k < 3; ++k) L.com_cost[k] = P.com_cost[0][k];
    L.com_gain = P.com_gain[0]; L.com_lm = P.com_lm[0];
    double mtot = 0.0;
    std::vector<double> wsum(3 * (nl > 0 ? nl : 1), 0.0);        // Σ m·(centre of mass in the link frame) per link
    for (int b = 1; b < m.nbody; ++b) {
      if (!in_robot[b]) continue;
      const double mb = m.body_mass[b];
      mtot += mb;
      // the body's centre of mass in the frame of its link (its own frame, or through the folded jointless chain) — or in the world
      Xf at = ident;
      if (m.body_jntnum[b] == 0) at = fold[b];
      const Xf cw = compose(at, &m.body_ipos[3 * b], ident.q);
      const int a = link_of[b];
      if (a < 0) { for (int k = 0; k < 3; ++k) L.com_static[k] += mb * cw.p[k]; continue; }
      L.link_mass[a] += mb;
      for (int k = 0; k < 3; ++k) wsum[3 * a + k] += mb * cw.p[k];
    }
    if (!(mtot > 0.0)) return 0;
    L.com_minv = 1.0 / mtot;
    for (int a = 0; a < nl; ++a) {
      for (int k = 0; k < 3; ++k) L.link_ipos[a][k] = L.link_mass[a] > 0.0 ? wsum[3 * a + k] / L.link_mass[a] : 0.0;
      // links are in body order (depth first): the subtree of a link is the range up to the next link that is not below it
      int last = a;
      for (int c = a + 1; c < nl; ++c) {
        int up = L.link[c].parent;
        while (up > a) up = L.link[up].parent;
        if (up != a) break;
        last = c;
      }
      L.link_last[a] = last;
      for (int c = a; c <= last; ++c) L.link_stmass[a] += L.link_mass[c];
    }
    for (int dd = 0; dd < m.nv; ++dd) if (L.dof_link[dd] < 0) return 0;     // (every dof of the robot moves mass: all need their link)
  }
  for (int t = 0; t < P.n_frame; ++t) {
    LaneFrame& f = L.frame[t];
    f.link = link_of[ft[t].body];
    f.chain = (uint32_t)ft[t].dof_mask;
    f.rowmask = ft[t].rowmask;
    const Xf fl = folded[ft[t].body] ? compose(fold[ft[t].body], ft[t].lpos, ft[t].lquat) : compose(ident, ft[t].lpos, ft[t].lquat);
    for (int i = 0; i < 3; ++i) f.lpos[i] = fl.p[i];
    for (int i = 0; i < 4; ++i) f.lquat[i] = fl.q[i];
    for (int i = 0; i < 6; ++i) f.cost[i] = ft[t].cost[i];
    f.gain = ft[t].gain; f.lm_damping = ft[t].lm_damping;
    if (ft[t].relative) {
      auto& r = L.rel[t];
      r.relative = 1;
      r.root_link = link_of[ft[t].root_body];
      r.rchain = (uint32_t)ft[t].root_mask;
      const Xf rl = folded[ft[t].root_body] ? compose(fold[ft[t].root_body], ft[t].root_lpos, ft[t].root_lquat)
                                             : compose(ident, ft[t].root_lpos, ft[t].root_lquat);
      for (int i = 0; i < 3; ++i) r.rlpos[i] = rl.p[i];
      for (int i = 0; i < 4; ++i) r.rlquat[i] = rl.q[i];
    }
  }
  for (int t = 0; t < P.n_posture; ++t) {
    for (int dd = 0; dd < m.nv; ++dd)      // (free-joint dofs: error and Jacobian column are zero, posture_task.py:115-116,139-141)
      L.posture_cost[t][dd] = m.jnt_type[m.dof_jntid[dd]] == JNT_FREE ? 0.0 : pcost[t * 64 + dd];
    L.posture_gain[t] = P.posture_gain[t]; L.posture_lm[t] = P.posture_lm[t];
  }
  for (int t = 0; t < kMaxBoxTerms; ++t)
    for (int dd = 0; dd < kLaneDescDofs2; ++dd) { L.cfg_lower[t][dd] = -inf; L.cfg_upper[t][dd] = inf; L.vel_limit[t][dd] = inf; }
  for (int t = 0; t < P.n_cfg; ++t) {
    L.cfg_gain[t] = P.cfg_gain[t];
    for (int dd = 0; dd < m.nv; ++dd) { L.cfg_lower[t][dd] = clo[t * 64 + dd]; L.cfg_upper[t][dd] = chi[t * 64 + dd]; }
  }
  for (int t = 0; t < P.n_vel; ++t)
    for (int dd = 0; dd < m.nv; ++dd) L.vel_limit[t][dd] = vlim[t * 64 + dd];
  if (has_free || com || has_relative || m.nv > 16 || nl > 16) return 32;                                     // (32: the row kernel on two DPP rows per problem)
  return m.nv <= 4 ? 4 : (m.nv <= 6 ? 6 : (m.nv == 7 ? 7 : (m.nv == 8 ? 8 : 16)));   // (16: the row kernel only)
}

// One create: the inputs, the plan being filled and the error text.
struct Ctx {
  const HostModel& m;
  const MkhProblemDesc& d;
  const int diag, max_batch, num_cus;
  const PlanSwitches& sw;
  ProblemPlan& pl;
  const Fail fail;
};

// pairs with an analytic routine (collide_dev.h) ...
bool analytic(int a, int b) {
  if (a > b) { int x = a; a = b; b = x; }
  return (a == PLAN_GEOM_CAPSULE && b == PLAN_GEOM_CAPSULE) || (a == PLAN_GEOM_SPHERE && b == PLAN_GEOM_SPHERE) ||
         (a == PLAN_GEOM_SPHERE && b == PLAN_GEOM_CAPSULE) || (a == PLAN_GEOM_PLANE && (b == PLAN_GEOM_SPHERE || b == PLAN_GEOM_CAPSULE)) ||
         (b == PLAN_GEOM_BOX && (a == PLAN_GEOM_PLANE || a == PLAN_GEOM_SPHERE || a == PLAN_GEOM_CAPSULE || a == PLAN_GEOM_BOX)) ||
         (b == PLAN_GEOM_CYLINDER && (a == PLAN_GEOM_PLANE || a == PLAN_GEOM_SPHERE || a == PLAN_GEOM_CAPSULE));
}
// ... and the ones that go through the general convex routine (convex_dev.h): cylinder–box, cylinder–cylinder,
// ellipsoid against any primitive, and every pair with a mesh geom (its hull: plane–mesh analytically)
bool convex(int a, int b) {
  if (a > b) { int x = a; a = b; b = x; }
  const bool cb = b == PLAN_GEOM_SPHERE || b == PLAN_GEOM_CAPSULE || b == PLAN_GEOM_ELLIPSOID || b == PLAN_GEOM_CYLINDER || b == PLAN_GEOM_BOX ||
                  b == PLAN_GEOM_MESH;
  return cb && (a == PLAN_GEOM_PLANE ? (b == PLAN_GEOM_ELLIPSOID || b == PLAN_GEOM_MESH) : (a >= PLAN_GEOM_SPHERE && a <= PLAN_GEOM_MESH));
}
// bounding spheres for the cull pass of problems with more than one wavefront of pairs (mkh_types.h PairCull)
double rbound(const HostModel& m, int g) {
  const double* sz = &m.geom_size[3 * g];
  switch (m.geom_type[g]) {
    case PLAN_GEOM_SPHERE: return sz[0];
    case PLAN_GEOM_CAPSULE: return sz[0] + sz[1];
    case PLAN_GEOM_ELLIPSOID: return std::fmax(sz[0], std::fmax(sz[1], sz[2]));
    case PLAN_GEOM_CYLINDER: return std::hypot(sz[0], sz[1]);
    case PLAN_GEOM_BOX: return std::sqrt(sz[0] * sz[0] + sz[1] * sz[1] + sz[2] * sz[2]);
    case PLAN_GEOM_MESH: {
      const int k = m.geom_dataid[g];
      double r2 = 0.0;
      if (k < 0 || m.h_mesh_vert.empty()) return kInf;
      for (int v = 0; v < m.mesh_vertnum[k]; ++v) {
        const double* x = &m.h_mesh_vert[3 * ((size_t)m.mesh_vertadr[k] + v)];
        r2 = std::fmax(r2, x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
      }
      return std::sqrt(r2);
    }
    default: return kInf;                                 // planes (and anything unbounded): never culled
  }
}

// a task's frame as (body, local pose)
int32_t resolve_frame(const Ctx& c, int t, int ftype, int fid, int32_t& body, const double*& lp, const double*& lq) {
  static const double zero3[3] = {0, 0, 0}, ident4[4] = {1, 0, 0, 0};
  const HostModel& m = c.m;
  if (ftype == MKH_FRAME_BODY) {
    if (fid < 0 || fid >= m.nbody) return c.fail(MKH_E_INVALID, "frame task %d: body id %d out of range", t, fid);
    body = fid; lp = zero3; lq = ident4;
  } else if (ftype == MKH_FRAME_SITE) {
    if (fid < 0 || fid >= m.nsite) return c.fail(MKH_E_INVALID, "frame task %d: site id %d out of range", t, fid);
    body = m.site_bodyid[fid]; lp = &m.site_pos[3 * fid]; lq = &m.site_quat[4 * fid];
  } else if (ftype == MKH_FRAME_GEOM) {
    if (fid < 0 || fid >= m.ngeom) return c.fail(MKH_E_INVALID, "frame task %d: geom id %d out of range", t, fid);
    body = m.geom_bodyid[fid]; lp = &m.geom_pos[3 * fid]; lq = &m.geom_quat[4 * fid];
  } else {
    return c.fail(MKH_E_INVALID, "frame task %d: unsupported frame type %d", t, ftype);
  }
  return MKH_OK;
}

// Everything that refuses a descriptor by what the caller wrote into it, in the order the tables below walk it.
int32_t validate(const Ctx& c) {
  const HostModel& m = c.m;
  const MkhProblemDesc& d = c.d;
  const auto& fail = c.fail;
  if (c.diag & ~(MKH_DIAG_NO_WIDE_REDO | MKH_DIAG_NO_TIGHT_REDO | MKH_DIAG_NO_COLD_REFINE | MKH_DIAG_NO_PAIR_CULL))
    return fail(MKH_E_INVALID, "unknown MKH_DIAG_* bits 0x%x", c.diag);
  if (c.max_batch < 1) return fail(MKH_E_INVALID, "max_batch must be >= 1");
  if (d.n_frame_tasks > kMaxFrameTasks) return fail(MKH_E_LIMIT, "at most %d frame tasks", kMaxFrameTasks);
  if (d.n_posture_tasks > kMaxPostureTasks) return fail(MKH_E_LIMIT, "at most %d posture tasks", kMaxPostureTasks);
  if (d.n_com_tasks > kMaxComTasks) return fail(MKH_E_LIMIT, "at most %d CoM tasks", kMaxComTasks);
  if (d.n_dense_tasks < 0 || d.n_dense_tasks > kMaxDenseTasks) return fail(MKH_E_LIMIT, "at most %d dense (plugin) tasks", kMaxDenseTasks);
  if (d.n_dense_limit_rows < 0) return fail(MKH_E_INVALID, "n_dense_limit_rows must be >= 0");
  if (d.n_configuration_limits > kMaxBoxTerms || d.n_velocity_limits > kMaxBoxTerms)
    return fail(MKH_E_LIMIT, "at most %d configuration and %d velocity limits", kMaxBoxTerms, kMaxBoxTerms);
  for (int t = 0; t < d.n_frame_tasks; ++t) {
    const MkhFrameTaskDesc& s = d.frame_tasks[t];
    int32_t body = 0;
    const double *lp = nullptr, *lq = nullptr;
    if (resolve_frame(c, t, s.frame_type, s.frame_id, body, lp, lq) != MKH_OK) return MKH_E_INVALID;
    if (s.root_type >= 0 && resolve_frame(c, t, s.root_type, s.root_id, body, lp, lq) != MKH_OK) return MKH_E_INVALID;
    for (int k = 0; k < 6; ++k)
      if (!(s.cost[k] >= 0.0)) return fail(MKH_E_INVALID, "frame task %d: cost must be >= 0", t);
  }
  for (int t = 0; t < d.n_dense_tasks; ++t) {
    const MkhDenseTaskDesc& s = d.dense_tasks[t];
    if (s.k < 1 || !s.cost) return fail(MKH_E_INVALID, "dense task %d: k must be >= 1 and cost non-null", t);
    if (!(s.gain >= 0.0 && s.gain <= 1.0) || !(s.lm_damping >= 0.0))
      return fail(MKH_E_INVALID, "dense task %d: gain must be in [0, 1] and lm_damping >= 0", t);
    for (int r = 0; r < s.k; ++r)
      if (!(s.cost[r] >= 0.0)) return fail(MKH_E_INVALID, "dense task %d: cost must be >= 0", t);
  }
  for (int t = 0; t < d.n_configuration_limits; ++t) {
    const MkhConfigurationLimitDesc& cl = d.configuration_limits[t];
    if (!(cl.gain > 0.0 && cl.gain <= 1.0)) return fail(MKH_E_INVALID, "configuration limit gain must be in (0, 1]");
    for (int k = 0; k < cl.n_indices; ++k) {
      const int dof = cl.indices[k];
      if (dof < 0 || dof >= m.nv) return fail(MKH_E_INVALID, "configuration limit: dof %d out of range", dof);
      if (m.jnt_type[m.dof_jntid[dof]] == JNT_FREE)
        return fail(MKH_E_INVALID, "configuration limit on free-joint dof %d (the reference skips free joints)", dof);
      if (m.jnt_type[m.dof_jntid[dof]] == JNT_BALL) {
        // the kernels rebuild a ball joint's bound as the quaternion (u, u, u, u) from the ONE value its dofs' table entries hold
        // (the range end, as the reference's constructor fills the joint's four qpos slots): anything else is not evaluated
        const int qa = m.jnt_qposadr[m.dof_jntid[dof]];
        for (int s = 1; s < 4; ++s)
          if (cl.lower[qa + s] != cl.lower[qa] || cl.upper[qa + s] != cl.upper[qa])
            return fail(MKH_E_INVALID, "configuration limit %d: lower / upper differ over the four qpos slots of the ball joint of dof %d "
                                       "(one value per ball joint, as the reference's constructor writes its range)", t, dof);
      }
    }
  }
  for (int t = 0; t < d.n_velocity_limits; ++t) {
    const MkhVelocityLimitDesc& v = d.velocity_limits[t];
    for (int k = 0; k < v.n_indices; ++k)
      if (v.indices[k] < 0 || v.indices[k] >= m.nv) return fail(MKH_E_INVALID, "velocity limit: dof %d out of range", v.indices[k]);
  }
  for (int t = 0; t < d.n_collision_limits; ++t) {
    const MkhCollisionLimitDesc& cl = d.collision_limits[t];
    for (int k = 0; k < cl.n_pairs; ++k) {
      const int g1 = cl.geom_id_pairs[2 * k], g2 = cl.geom_id_pairs[2 * k + 1];
      if (g1 < 0 || g2 < 0 || g1 >= m.ngeom || g2 >= m.ngeom) return fail(MKH_E_INVALID, "collision pair (%d,%d): geom id out of range", g1, g2);
      const int t1 = m.geom_type[g1], t2 = m.geom_type[g2];
      if (!analytic(t1, t2) && !convex(t1, t2))
        return fail(MKH_E_INVALID, "collision pair (%d,%d): geom types (%d,%d) are not supported (height fields)", g1, g2, t1, t2);
      for (int g : {g1, g2})
        if (m.geom_type[g] == PLAN_GEOM_MESH && (m.geom_dataid[g] < 0 || m.h_mesh_vert.empty()))
          return fail(MKH_E_INVALID, "collision pair (%d,%d): mesh geom %d has no hull in the model (geom_dataid / mesh_vert)", g1, g2, g);
    }
  }
  return MKH_OK;
}

// One value per dof of every PostureTask / ConfigurationLimit / VelocityLimit, rows `stride` apart: the lane tables of the
// wavefront kernels (64) and the plain arrays of the workgroup-per-problem kernel (nv) — `fill` = false leaves the defaults
// (a model beyond one wavefront has no lane tables).
void dof_tables(const Ctx& c, int stride, bool fill, std::vector<double>& pcost, std::vector<double>& clo, std::vector<double>& chi,
                std::vector<double>& vlim) {
  const HostModel& m = c.m;
  const MkhProblemDesc& d = c.d;
  const int np = d.n_posture_tasks, nc = d.n_configuration_limits, nl = d.n_velocity_limits;
  pcost.assign((size_t)(np ? np : 1) * stride, 0.0);
  clo.assign((size_t)(nc ? nc : 1) * stride, -kInf);
  chi.assign((size_t)(nc ? nc : 1) * stride, kInf);
  vlim.assign((size_t)(nl ? nl : 1) * stride, kInf);
  if (!fill) return;
  for (int t = 0; t < np; ++t)
    for (int i = 0; i < m.nv; ++i) pcost[(size_t)t * stride + i] = d.posture_tasks[t].cost[i];
  // box limits: per-dof lower/upper in joint coordinates (±inf = absent)
  for (int t = 0; t < nc; ++t) {
    const MkhConfigurationLimitDesc& cl = d.configuration_limits[t];
    for (int k = 0; k < cl.n_indices; ++k) {
      const int dof = cl.indices[k], qa = m.jnt_qposadr[m.dof_jntid[dof]];
      clo[(size_t)t * stride + dof] = cl.lower[qa];
      chi[(size_t)t * stride + dof] = cl.upper[qa];
    }
  }
  for (int t = 0; t < nl; ++t) {
    const MkhVelocityLimitDesc& v = d.velocity_limits[t];
    for (int k = 0; k < v.n_indices; ++k) {
      double& x = vlim[(size_t)t * stride + v.indices[k]];
      x = std::fmin(x, v.limit[k]);
    }
  }
}

// ---- 1. task rows: frames resolved to (body, local pose), rows of the tap layout and of the compact LDS layout
void plan_task_rows(Ctx& c) {
  const HostModel& m = c.m;
  const MkhProblemDesc& d = c.d;
  DeviceProblem& P = c.pl.dev;
  ProblemSelect& S = c.pl.sel;
  P.nq = m.nq; P.nv = m.nv; P.nbody = m.nbody; P.njnt = m.njnt; P.nrounds = m.nrounds;
  P.robot_root = 1;
  // (joint anchors at the body origins — the G1, most menagerie robots: the kinematics skip rotating the zero offset)
  P.jnt_pos_zero = 1;
  for (double x : m.jnt_pos) if (x != 0.0) P.jnt_pos_zero = 0;
  P.n_frame = d.n_frame_tasks; P.n_posture = d.n_posture_tasks; P.n_com = d.n_com_tasks;
  P.n_cfg = d.n_configuration_limits; P.n_vel = d.n_velocity_limits;
  int row = 0, jrows = 0;
  std::vector<FrameTaskDev>& ft = c.pl.ft;
  ft.resize(d.n_frame_tasks);
  for (int t = 0; t < d.n_frame_tasks; ++t) {
    const MkhFrameTaskDesc& s = d.frame_tasks[t];
    FrameTaskDev& f = ft[t];
    memset(&f, 0, sizeof f);
    const double *lp = nullptr, *lq = nullptr;
    (void)resolve_frame(c, t, s.frame_type, s.frame_id, f.body, lp, lq);
    for (int k = 0; k < 3; ++k) f.lpos[k] = lp[k];
    for (int k = 0; k < 4; ++k) f.lquat[k] = lq[k];
    if (s.root_type >= 0) {
      f.relative = 1;
      S.has_relative = true;
      (void)resolve_frame(c, t, s.root_type, s.root_id, f.root_body, lp, lq);
      for (int k = 0; k < 3; ++k) f.root_lpos[k] = lp[k];
      for (int k = 0; k < 4; ++k) f.root_lquat[k] = lq[k];
      f.root_mask = m.big ? 0ull : m.chain_mask(f.root_body);
    }
    for (int k = 0; k < 6; ++k) f.cost[k] = s.cost[k];
    f.gain = s.gain; f.lm_damping = s.lm_damping;
    f.dof_mask = m.big ? 0ull : m.chain_mask(f.body);
    f.row0 = row; row += 6;
    f.any_ori = (s.cost[3] != 0.0 || s.cost[4] != 0.0 || s.cost[5] != 0.0) ? 1 : 0;
    f.rowmask = 0;
    for (int k = 0; k < 6; ++k) if (s.cost[k] != 0.0) f.rowmask |= 1 << k;
    f.jrow0 = jrows;
    jrows += __builtin_popcount(f.rowmask);
  }
  S.frame_w.assign(2 * (size_t)d.n_frame_tasks, 0.0);
  for (int t = 0; t < d.n_frame_tasks; ++t) {
    if (ft[t].relative) continue;
    S.frame_w[t] = (ft[t].rowmask & 7) ? 1.0 : 0.0;
    S.frame_w[d.n_frame_tasks + t] = ft[t].any_ori ? 1.0 : 0.0;
  }
  for (int t = 0; t < d.n_posture_tasks; ++t) {
    P.posture_gain[t] = d.posture_tasks[t].gain; P.posture_lm[t] = d.posture_tasks[t].lm_damping;
    P.posture_row0[t] = row; row += m.nv;
  }
  for (int t = 0; t < d.n_com_tasks; ++t) {
    for (int k = 0; k < 3; ++k) P.com_cost[t][k] = d.com_tasks[t].cost[k];
    P.com_gain[t] = d.com_tasks[t].gain; P.com_lm[t] = d.com_tasks[t].lm_damping;
    P.com_row0[t] = row; row += 3;
    P.com_rowmask[t] = 0;
    for (int k = 0; k < 3; ++k) if (d.com_tasks[t].cost[k] != 0.0) P.com_rowmask[t] |= 1 << k;
    P.com_jrow0[t] = jrows;
    jrows += __builtin_popcount(P.com_rowmask[t]);
  }
  // plugin route: caller-defined tasks as dense rows (tap rows follow the built-in ones)
  P.n_dense_tasks = d.n_dense_tasks;
  P.dense_tap_row0 = row;
  for (int t = 0; t < d.n_dense_tasks; ++t) {
    const MkhDenseTaskDesc& s = d.dense_tasks[t];
    P.dense_row0[t] = (int)c.pl.dcost.size(); P.dense_k[t] = s.k; P.dense_lm[t] = s.lm_damping;
    for (int r = 0; r < s.k; ++r) {
      c.pl.dcost.push_back(s.cost[r]);
      c.pl.dwgain.push_back(s.cost[r] * -s.gain);
    }
    row += s.k;
  }
  P.n_dense_rows = (int)c.pl.dcost.size();
  P.n_dense_limit_rows = d.n_dense_limit_rows;
  P.dense_box = d.dense_limit_box ? 1 : 0;
  P.n_rows_tap = row;
  P.n_jrows = jrows;
}

// ---- 2. box limits and posture costs as lane tables
void plan_box_limits(Ctx& c) {
  for (int t = 0; t < c.d.n_configuration_limits; ++t) c.pl.dev.cfg_gain[t] = c.d.configuration_limits[t].gain;
  dof_tables(c, 64, !c.m.big, c.pl.pcost, c.pl.clo, c.pl.chi, c.pl.vlim);
}

// ---- 3. collision pairs and their bounding-sphere records
void plan_pairs(Ctx& c) {
  const HostModel& m = c.m;
  ProblemSelect& S = c.pl.sel;
  std::vector<CollisionPairDev>& pairs = c.pl.pairs;
  int n_cv = 0;
  for (int t = 0; t < c.d.n_collision_limits; ++t) {
    const MkhCollisionLimitDesc& cl = c.d.collision_limits[t];
    for (int k = 0; k < cl.n_pairs; ++k) {
      const int g1 = cl.geom_id_pairs[2 * k], g2 = cl.geom_id_pairs[2 * k + 1];
      CollisionPairDev cp;
      memset(&cp, 0, sizeof cp);
      const int t1 = m.geom_type[g1], t2 = m.geom_type[g2];
      cp.cv_slot = -1;
      if (!analytic(t1, t2) && convex(t1, t2)) { S.convex_pairs = true; cp.cv_slot = n_cv++; }
      long long vert[2] = {-1, -1};
      for (int side = 0; side < 2; ++side) {
        const int g = side ? g2 : g1;
        if (m.geom_type[g] != PLAN_GEOM_MESH) continue;
        const int km = m.geom_dataid[g];
        vert[side] = 3 * (long long)m.mesh_vertadr[km];
        (side ? cp.nvert2 : cp.nvert1) = m.mesh_vertnum[km];
      }
      c.pl.pair_vert.push_back(vert[0]); c.pl.pair_vert.push_back(vert[1]);
      c.pl.pair_geom.push_back(g1); c.pl.pair_geom.push_back(g2);
      cp.type1 = t1; cp.type2 = t2; cp.body1 = m.geom_bodyid[g1]; cp.body2 = m.geom_bodyid[g2];
      for (int i = 0; i < 3; ++i) { cp.size1[i] = m.geom_size[3 * g1 + i]; cp.size2[i] = m.geom_size[3 * g2 + i];
                                    cp.lpos1[i] = m.geom_pos[3 * g1 + i]; cp.lpos2[i] = m.geom_pos[3 * g2 + i]; }
      for (int i = 0; i < 4; ++i) { cp.lquat1[i] = m.geom_quat[4 * g1 + i]; cp.lquat2[i] = m.geom_quat[4 * g2 + i]; }
      if (!m.big) { cp.mask1 = m.chain_mask(cp.body1); cp.mask2 = m.chain_mask(cp.body2); }
      cp.gain = cl.gain; cp.dmin = cl.minimum_distance_from_collisions; cp.ddetect = cl.collision_detection_distance;
      cp.relax = cl.bound_relaxation;
      pairs.push_back(cp);
      PairCull pc;
      memset(&pc, 0, sizeof pc);
      pc.body1 = cp.body1; pc.body2 = cp.body2;
      for (int i = 0; i < 3; ++i) { pc.lpos1[i] = cp.lpos1[i]; pc.lpos2[i] = cp.lpos2[i]; }
      const double reach = (rbound(m, g1) + rbound(m, g2) + std::fmax(cp.ddetect, 0.0)) * (1.0 + 1e-9) + 1e-12;
      pc.reach2 = reach * reach;
      c.pl.culls.push_back(pc);
    }
  }
  c.pl.dev.n_pairs = (int)pairs.size();
  c.pl.n_cv = n_cv;                                  // (plan_convex_split keeps or zeroes it)
  S.simple_pairs = !pairs.empty();
  for (const auto& cp : pairs)
    for (int ty : {cp.type1, cp.type2})
      if (ty != PLAN_GEOM_PLANE && ty != PLAN_GEOM_SPHERE && ty != PLAN_GEOM_CAPSULE) S.simple_pairs = false;
}

// ---- 4. row cap and tableau size
int32_t plan_tableau(Ctx& c) {
  const HostModel& m = c.m;
  DeviceProblem& P = c.pl.dev;
  ProblemSelect& S = c.pl.sel;
  const int want = P.n_pairs + P.n_dense_limit_rows;          // half-space rows that can be active at once
  P.max_rows = want < (kWave - m.nv) ? want : (kWave - m.nv);
  if (c.sw.max_rows > 0 && c.sw.max_rows < P.max_rows) P.max_rows = c.sw.max_rows;   // (experiments)
  // LDS behind the per-problem ranges: h of every pair when pairs outnumber rows (row selection), then the expanding polytope's
  // workspace when some pair goes through the general convex routine (collision_phase: the same two terms)
  P.n_hsel = (P.n_pairs > P.max_rows ? lds_even(P.n_pairs) : 0) + (S.convex_pairs ? kConvexWsDoubles : 0);
  // the cull pass's candidate list (16-bit pair indices) when the pairs do not fit one trip of the wavefront
  S.use_cull = P.n_pairs > kWave && P.n_pairs < 65536 && !S.simple_pairs && !(c.diag & MKH_DIAG_NO_PAIR_CULL);
  if (S.use_cull) P.n_hsel += lds_even((P.n_pairs + 3) / 4);
  const int ntab = m.nv + P.max_rows;
  S.nt = size_class(ntab, 0);       // (ntab ≤ kWave by the cap on max_rows above: the largest build holds it)
  if (!S.nt) return c.fail(MKH_E_LIMIT, "no kernel variant with %d tableau rows", ntab);
  P.nt = S.nt;
  S.nt_full = S.nt < 32 ? 32 : S.nt;
  return MKH_OK;
}

// ---- 5. direct-start layouts
int32_t plan_direct_layouts(Ctx& c) {
  DeviceProblem& P = c.pl.dev;
  ProblemSelect& S = c.pl.sel;
  // Second LDS buffers for the next problem's inputs (ik_kernel.h "load inputs") only where they do not cost a
  // resident wave in the lean or the all-feature variant of this problem (the low-rank variant is checked below).
  auto lds_of = [&](int nt, bool pre) { return lds_bytes_of(P, nt, 0, kDirectFeat, false, pre); };
  P.prefetch = (waves_per_cu(S.nt, lds_of(S.nt, true)) == waves_per_cu(S.nt, lds_of(S.nt, false)) &&
                waves_per_cu(S.nt_full, lds_of(S.nt_full, true)) == waves_per_cu(S.nt_full, lds_of(S.nt_full, false))) ? 1 : 0;
  S.lds_bytes = lds_of(S.nt, P.prefetch != 0);
  if (S.lds_bytes > 64 * 1024) return c.fail(MKH_E_LIMIT, "problem needs %d bytes of LDS per wavefront (> 64 KiB)", S.lds_bytes);
  S.blocks_per_cu = waves_per_cu(S.nt, S.lds_bytes);
  S.lds_bytes_full = lds_of(S.nt_full, P.prefetch != 0);
  if (S.blocks_per_cu < 1) S.blocks_per_cu = 1;
  // 3 waves per SIMD: tableau sizes with a lean build on the TabW3 map, no half-space rows (the compact layout lets the
  // Jacobian rows reuse the body poses, which the collision phase still reads), and 12 wavefronts' LDS must fit the CU
  P.prefetch_w3 = 0;
  if (find_variant(S.nt, 0, 0, true) && P.max_rows == 0 && P.n_dense_rows == 0) {
    auto lds_w3 = [&](bool pre) { return lds_bytes_of(P, S.nt, 0, 0, true, pre); };
    if (waves_per_cu(S.nt, lds_w3(false), true) == 12) {
      P.prefetch_w3 = waves_per_cu(S.nt, lds_w3(true), true) == 12 ? 1 : 0;
      S.lds_bytes_w3 = lds_w3(P.prefetch_w3 != 0);
    }
  }
  return MKH_OK;
}

// ---- 6. direct start: Jacobian columns by (task, dof) pair lanes when they fit one wavefront
void plan_direct_pairs(Ctx& c) {
  DeviceProblem& P = c.pl.dev;
  const std::vector<FrameTaskDev>& ft = c.pl.ft;
  P.n_dpairs = 0;
  int n = 0;
  bool fits = true;
  for (size_t t = 0; t < ft.size() && fits; ++t) {
    const uint64_t cm = ft[t].dof_mask | (ft[t].relative ? ft[t].root_mask : 0ull);
    for (int k = 0; k < c.m.nv && fits; ++k)
      if ((cm >> k) & 1) {
        if (n >= kWave) { fits = false; break; }
        P.dpair_task[n] = (int16_t)t; P.dpair_dof[n] = (int16_t)k; ++n;
      }
  }
  if (fits) P.n_dpairs = n;
}

// The low-rank start's lane tables (ik_kernel.h wood_start): which column / row chunk of Jh·Jhᵀ a lane computes and over which
// dofs, the (task, dof) pair lanes of the Jacobian rows, the source of each residual's weighted error.  They depend on the
// tasks only — shared by the builds without rows and, round 6, the ones with half-space rows.  false: more than 256 pairs.
bool wood_tables(Ctx& c) {
  DeviceProblem& P = c.pl.dev;
  const std::vector<FrameTaskDev>& ft = c.pl.ft;
  const int nv = c.m.nv;
  // (column, row-chunk) lanes of the Jh·Jhᵀ product: rows 0..n_jrows (the last one is the rhs)
  const int groups = kWave / P.n_jrows;
  P.wood_rpc = (P.n_jrows + 1 + groups - 1) / groups;
  for (int l = 0; l < kWave; ++l) {
    const int ch = l / P.n_jrows;
    P.wood_col[l] = ch < groups ? l % P.n_jrows : -1;
    P.wood_row0[l] = ch < groups ? ch * P.wood_rpc : 0;
    P.wood_mask[l] = 0;
    if (ch < groups)
      for (size_t t = 0; t < ft.size(); ++t)
        if (l % P.n_jrows >= ft[t].jrow0 && l % P.n_jrows < ft[t].jrow0 + __builtin_popcount(ft[t].rowmask & 63))
          P.wood_mask[l] = ft[t].dof_mask;
  }
  // Jacobian columns by (task, dof) pair lanes; source of each residual's weighted error
  P.n_jpairs = 0;
  for (size_t t = 0; t < ft.size(); ++t) {
    for (int k = 0; k < nv; ++k)
      if ((ft[t].dof_mask >> k) & 1) {
        if (P.n_jpairs >= 256) return false;
        P.jpair_task[P.n_jpairs] = (int16_t)t; P.jpair_dof[P.n_jpairs] = (int16_t)k; ++P.n_jpairs;
      }
    int cnt = 0;
    for (int r = 0; r < 6; ++r)
      if ((ft[t].rowmask >> r) & 1) { P.mu_src[ft[t].jrow0 + cnt] = (int16_t)(t * 64 + 30 + r); ++cnt; }
  }
  // ComTask rows: dense over the robot's dofs; their weighted error is computed on the device (mu_src < 0)
  for (int t = 0; t < P.n_com; ++t) {
    int cnt = 0;
    for (int r = 0; r < 3; ++r)
      if ((P.com_rowmask[t] >> r) & 1) { P.mu_src[P.com_jrow0[t] + cnt] = (int16_t)(-1 - 3 * t - r); ++cnt; }
    for (int l = 0; l < kWave; ++l)
      if (P.wood_col[l] >= P.com_jrow0[t] && P.wood_col[l] < P.com_jrow0[t] + cnt)
        P.wood_mask[l] = nv >= 64 ? ~0ull : ((1ull << nv) - 1ull);
  }
  // What a product lane used to work out of these tables in every solve.  Its dofs as a list: ascending, as the walk over
  // the bits of wood_mask takes them (the order of the sums, hence every bit of S, stays), one byte each; every lane walks
  // wood_trip entries, the longest list, a shorter one padded with a dof off its chain — that entry of its Jh row is the
  // filled zero, and +0·b leaves a sum that started at +0 as it is.  No lists (wood_trip = 0, the lanes walk the mask)
  // when a chain has more than kWoodList dofs or a shorter lane has no dof to pad with.
  // Its stores: rows [wood_row0, +wood_rpc) below n_jrows go to S, row n_jrows — entry wood_jrhs of the one chunk that
  // holds it — to w.
  P.wood_trip = 0;
  P.wood_jrhs = P.n_jrows % P.wood_rpc;
  bool lists = true;
  for (int l = 0; l < kWave; ++l) {
    for (int i = 0; i < 4; ++i) P.wood_list[l][i] = 0;
    if (P.wood_col[l] < 0) continue;
    const int len = __builtin_popcountll(P.wood_mask[l]);
    if (len > kWoodList) lists = false;
    P.wood_trip = len > P.wood_trip ? len : P.wood_trip;
  }
  for (int l = 0; l < kWave && lists; ++l) {
    if (P.wood_col[l] < 0) continue;
    int n = 0, pad = -1;
    for (int k = 0; k < 64; ++k) {
      if ((P.wood_mask[l] >> k) & 1) { P.wood_list[l][n >> 2] |= (uint32_t)k << (8 * (n & 3)); ++n; }
      else if (pad < 0 && k < nv) pad = k;
    }
    if (n < P.wood_trip && pad < 0) lists = false;
    for (; n < P.wood_trip && lists; ++n) P.wood_list[l][n >> 2] |= (uint32_t)pad << (8 * (n & 3));
  }
  if (!lists) P.wood_trip = 0;
  return true;
}

// what the low-rank start's stability criterion compares (plan_launch(): damping + the smallest posture diagonal against the largest
// task cost²)
void wood_scales(Ctx& c) {
  const HostModel& m = c.m;
  const DeviceProblem& P = c.pl.dev;
  ProblemSelect& S = c.pl.sel;
  double mn = __builtin_huge_val();
  for (int i = 0; i < m.nv; ++i) {
    double dsum = 0.0;
    for (int t = 0; t < c.d.n_posture_tasks; ++t) {
      // free-joint dofs carry no posture term (posture_task.py:115-116,139-141)
      const int jt = m.jnt_type[m.dof_jntid[i]];
      if (jt != 0) dsum += c.pl.pcost[t * 64 + i] * c.pl.pcost[t * 64 + i];
    }
    mn = dsum < mn ? dsum : mn;
  }
  S.wood_min_diag = mn;
  S.wood_max_cost2 = 0.0;
  for (const auto& f : c.pl.ft) for (int k = 0; k < 6; ++k) S.wood_max_cost2 = fmax(S.wood_max_cost2, f.cost[k] * f.cost[k]);
  for (int t = 0; t < P.n_com; ++t) for (int k = 0; k < 3; ++k) S.wood_max_cost2 = fmax(S.wood_max_cost2, P.com_cost[t][k] * P.com_cost[t][k]);
}

// ---- 7./8. low-rank start: whether it applies and pays, its layouts on the three register maps, its tables
void plan_wood(Ctx& c) {
  const HostModel& m = c.m;
  DeviceProblem& P = c.pl.dev;
  ProblemSelect& S = c.pl.sel;
  if (!(P.n_jrows > 0 && P.n_pairs == 0 && !S.has_relative && P.n_dense_rows == 0 && P.n_dense_limit_rows == 0 && P.n_jrows <= kMuBig))
    return;
  // (NT = NR: the task residuals are eliminated outside the tableau, one column of [S | Jh] per lane — wood_start; the
  //  S columns sit on lanes [NR, NR + n_μ) or, when those do not exist, on lanes [0, n_μ) in a second register set)
  int cand = 0;
  for (int v = size_class(m.nv, F_WOOD, true); v && !cand; v = size_class(v + 1, F_WOOD, true))
    if (v + P.n_jrows <= kWave || P.n_jrows <= v) cand = v;
  const bool big = P.n_jrows > kMu || cand + P.n_jrows > kWave;
  // When it pays.  Fewer task rows than dofs by a margin — half, three quarters for humanoid-size tableaus — measured in
  // rounds 1-2 on arms, hands and the G1; round 4 (tools/bench_wood_criterion.py, H1 / Go1 / Spot / Allegro / Shadow with
  // 12-18 rows on 18-25 dofs): whenever the small elimination applies (≤ kMu rows, S columns on lanes of their own) the
  // low-rank start wins by 1.15-1.38 x up to rows = dofs; the large one (> kMu rows) loses beyond three quarters
  // (Shadow 21 / 24: 0.57 x, H1 24 / 25: 0.93 x) and keeps the old margin.
  const bool pays = 2 * P.n_jrows <= m.nv || (m.nv >= 32 && 4 * P.n_jrows <= 3 * m.nv) ||
                    (!big && m.nv >= 16 && P.n_jrows <= m.nv) || c.sw.wood_always;
  if (cand && pays) { S.wood_nt = cand; S.wood_nr = cand; }
  if (!S.wood_nt) return;
  S.wood_big = P.n_jrows > kMu || S.wood_nr + P.n_jrows > kWave;
  // (two-waves map: plain or compact layout; one-more-wave map: always compact, one pivot buffer on the F_COM builds)
  auto lds_wood = [&](bool pre, bool compact) { return lds_bytes_of(P, S.wood_nt, S.wood_nr, F_WOOD, false, pre, compact); };
  auto lds_wood_w3 = [&](int feat, bool pre) { return lds_bytes_of(P, S.wood_nt, S.wood_nr, feat, true, pre); };
  // 2-waves map: the plain layout, or — when that would cost a resident wave and the pair lanes need one pass only (the
  // compact layout lets the Jacobian rows overwrite the task blocks) — the compact one
  P.wood_compact = 0; P.prefetch_wc = 0;
  P.wood_refine = (c.diag & MKH_DIAG_NO_COLD_REFINE) ? 0 : 1;
  if (waves_per_cu(S.wood_nt, lds_wood(false, false)) < waves_per_cu(S.wood_nt, 1) && P.n_jrows > 0) {
    int n_jp = 0;
    for (size_t t = 0; t < c.pl.ft.size(); ++t) n_jp += __builtin_popcountll(c.pl.ft[t].dof_mask);
    if (n_jp <= kWave && waves_per_cu(S.wood_nt, lds_wood(false, true)) > waves_per_cu(S.wood_nt, lds_wood(false, false))) {
      P.wood_compact = 1;
      P.prefetch_wc = waves_per_cu(S.wood_nt, lds_wood(true, true)) == waves_per_cu(S.wood_nt, lds_wood(false, true)) ? 1 : 0;
    }
  }
  S.wood_lds_bytes = P.wood_compact ? lds_wood(P.prefetch_wc != 0, true) : lds_wood(P.prefetch != 0, false);
  if (!wood_tables(c)) S.wood_nt = 0;
  if (S.wood_lds_bytes * 8 > 160 * 1024) S.wood_nt = 0;      // would cost residency
  // 3 waves per SIMD (compact layout: the Jacobian rows overwrite the task blocks, so the pair lanes need one pass)
  P.prefetch_w3w = 0;
  if (find_variant(S.wood_nt, S.wood_nr, F_WOOD, true) && P.n_jpairs <= kWave && P.n_com == 0 && !S.wood_big) {
    const int full = waves_per_cu(S.wood_nt, 1, true);     // 16 waves per CU for NT ≤ 24, else 12
    if (waves_per_cu(S.wood_nt, lds_wood_w3(F_WOOD, false), true) == full) {
      P.prefetch_w3w = waves_per_cu(S.wood_nt, lds_wood_w3(F_WOOD, true), true) == full ? 1 : 0;
      S.wood_lds_bytes_w3 = lds_wood_w3(F_WOOD, P.prefetch_w3w != 0);
    }
  }
  // ... and four (the product-form build on TabW4<44>, one problem per workgroup: everything that is dead after the pair lanes
  // in one union, lds_layout.h build_lds_layout_w4p).  Sixteen wavefronts per CU by registers (128 VGPRs), so the layout has to
  // fit 8 of the CU's 128 LDS granules; 9 would be 14 wavefronts, uneven SIMDs — the problem then stays on the three-waves build.
  S.wood_lds_bytes_w4 = 0;
  if (S.wood_lds_bytes_w3 && S.wood_nt == 44 && P.n_com == 0 && !S.wood_big && find_variant(44, 44, F_WOOD, true, true, true)) {
    const int bytes = build_lds_layout_w4p(P, S.wood_nr).total * (int)sizeof(double);
    if (128 / ((bytes + 1279) / 1280) >= 16) S.wood_lds_bytes_w4 = bytes;
  }
  // ... and the F_COM builds of a humanoid-size robot (ComTask rows and / or up to 24 task rows: `44_36_r44_w3`, round 5).
  // Their 25 rows of Jh take 8.8 KB of the compact layout — 15.4 KB for the G1 full example, 10 wavefronts per CU instead
  // of 8 — so the bar is "more resident wavefronts than the two-waves map", not all twelve.
  if (!c.sw.no_com_w3 && find_variant(S.wood_nt, S.wood_nr, F_WOOD | F_COM, true) && P.n_jpairs <= kWave && (P.n_com > 0 || S.wood_big)) {
    const int two = waves_per_cu(S.wood_nt, 1, false);     // 8
    const int w = waves_per_cu(S.wood_nt, lds_wood_w3(F_WOOD | F_COM, false), true);
    if (w >= two + 2) {                                   // (nine per CU — 3 + 2 + 2 + 2 — measured SLOWER than eight: 1.51 vs 1.44 ms)
      P.prefetch_w3w = waves_per_cu(S.wood_nt, lds_wood_w3(F_WOOD | F_COM, true), true) == w ? 1 : 0;
      S.wood_lds_bytes_w3 = lds_wood_w3(F_WOOD | F_COM, P.prefetch_w3w != 0);
    }
  }
  wood_scales(c);
}

int woodr_bytes(const DeviceProblem& D, bool pre) { return lds_bytes_of(D, 48, 48, F_WOOD | F_COLL, false, pre); }

// ---- 9. low-rank start WITH half-space rows (round 6; ik_kernel.h wood_start "half-space rows"): a collision problem whose
// tasks qualify for the low-rank start keeps it — every contact row is one more column of the n_μ-step elimination instead of
// the reason for nv single pivots on the whole tableau (47 % of `g1_coll`).  Analytic pair sets (FEAT 8 → 40), frame + posture
// tasks, at most kMu task rows, one pass of (task, dof) pair lanes (the Jacobian rows overwrite the task blocks in LDS) and at most
// 8 half-space rows per instance (the rows' Gram entries wait in the contact table); a 48-row tableau (plan_tight_rows below).
void plan_wood_rows(Ctx& c) {
  DeviceProblem& P = c.pl.dev;
  ProblemSelect& S = c.pl.sel;
  if (P.n_jrows > 0 && P.n_jrows <= kMu && P.n_pairs > 0 && !S.has_relative && P.n_com == 0 && P.n_dense_rows == 0 &&
      P.n_dense_limit_rows == 0 && !P.dense_box && !S.simple_pairs && !S.convex_pairs) {
    if (wood_tables(c) && P.n_jpairs <= kWave) { S.woodr_tables = true; wood_scales(c); }
  }
  if (S.woodr_tables && S.nt == 48 && P.max_rows <= 8) {
    P.prefetch_wc = waves_per_cu(48, woodr_bytes(P, true)) == waves_per_cu(48, woodr_bytes(P, false)) ? 1 : 0;
    S.woodr_lds = woodr_bytes(P, P.prefetch_wc != 0);
  }
}

// ---- 10. the lane / row kernels' descriptor
void plan_lane(Ctx& c) {
  ProblemPlan& pl = c.pl;
  ProblemSelect& S = pl.sel;
  LaneProblem2& lp = pl.lane;
  const int small_cls = build_lane_problem(c.m, pl.dev, pl.ft, pl.pcost, pl.clo, pl.chi, pl.vlim, S.has_relative, lp);
  pl.lane_class = small_cls;
  S.lane_nv = small_cls <= 8 ? small_cls : 0;
  S.quad_nt = small_cls ? (small_cls <= 8 ? 8 : (small_cls == 32 ? 32 : 16)) : 0;
  if (c.sw.no_pair_rows && S.quad_nt == 32) S.quad_nt = 0;   // (A/B switch: 17 … 32-dof robots back on the wavefront kernel)
  // (the two-row loop carries a free joint's quaternion on the link of its rotation; a free body on no task chain — the loose
  //  object of a hand scene — has no link, and its loops stay on the wavefront kernel, which integrates every joint)
  if (small_cls == 32 && lp.nq != lp.nv) {
    bool linked = false;
    for (int k = 0; k < lp.nlink; ++k) linked = linked || lp.link[k].jtype == JNT_BALL;
    S.quad_loop_ok = linked;
  }
  if (small_cls) {
    S.lane_lds = lane_lds_bytes(lp.nlink);
    bool ident = true;
    for (int dd = 0; dd < lp.nv; ++dd) ident = ident && lp.dof_qadr[dd] == dd;
    S.lane_dims = LaneDims{lp.nq, lp.nv, lp.nlink, lp.n_frame, lp.n_posture, lp.n_cfg, lp.n_vel, ident ? 1 : 0};
  }
}

// ---- 11. Tight rows: a hand with 40 capsule pairs has ≈17 contacts inside the detection distance at a time, but 40 rows put it
// on the 64-row tableau (128 pinned VGPRs, 23 KB of LDS: 7 wavefronts per CU).  With 48 − nv rows it runs on the 48-row
// build — Shadow config 4: 0.398 → 0.343 ms — and the rare instance with a violated dropped contact is solved again on
// the full-row build (launch()).
void plan_tight_rows(Ctx& c) {
  const DeviceProblem& P0 = c.pl.dev;
  ProblemSelect& S = c.pl.sel;
  const int nv = c.m.nv, cap = 48 - nv;
  // Round 5: the same for pair sets with boxes, cylinders, ... (the analytic collision build) — a humanoid-size robot reserves
  // 64 − nv rows, which costs the 64-row build a resident wavefront or two in LDS: G1 with 46 pairs (21 rows, 24.6 KB: 6
  // wavefronts per CU) 0.757 → ≈ 0.60 ms with 5 rows on the 48-row build.  Few contacts are in range at a time when
  // collision avoidance works; when many are, the cost is the two launches (MKH_FLAG_FULL_ROWS pins the full-row build).
  //  Humanoid-size robots only (32 dofs and up): ALOHA (16 dofs, 48 rows reserved, 1 104 pairs) measures 2.26 → 2.53 ms this
  //  way — its full build is not short of wavefronts, and the instances that overflow 32 rows walk the pair list twice.
  const bool generic = !S.simple_pairs && !S.convex_pairs && P0.n_pairs > 0 && nv >= 32 && cap >= 4 && !c.sw.no_tight_generic;
  if (c.sw.no_tight_rows || !(S.simple_pairs ? cap >= 16 : generic) || P0.n_dense_limit_rows != 0 || P0.n_dense_rows != 0 || P0.dense_box ||
      S.nt != 64 || P0.n_pairs <= cap)
    return;
  DeviceProblem& T = c.pl.dev_tight;
  T = P0;
  T.max_rows = cap;
  T.n_hsel = lds_even(T.n_pairs) + (S.use_cull ? lds_even((T.n_pairs + 3) / 4) : 0);
  T.nt = 48;
  auto lds_t = [&](bool pre) { return lds_bytes_of(T, 48, 0, kDirectFeat, false, pre); };
  T.prefetch = waves_per_cu(48, lds_t(true)) == waves_per_cu(48, lds_t(false)) ? 1 : 0;
  S.nt_tight = 48;
  S.lds_tight = lds_t(T.prefetch != 0);
  if (S.woodr_tables && T.max_rows <= 8) {               // the tight launch with the low-rank start (round 6)
    T.prefetch_wc = waves_per_cu(48, woodr_bytes(T, true)) == waves_per_cu(48, woodr_bytes(T, false)) ? 1 : 0;
    S.woodr_lds_tight = woodr_bytes(T, T.prefetch_wc != 0);
  }
  c.pl.tight = true;
}

// ---- 12. The descriptor of the workgroup-per-problem kernel (wide_kernel.h): plain arrays over bodies / joints / dofs (no 64-wide
// lane tables; the model's own: HostModel), LDS offsets, and the per-workgroup slice of device memory (weighted Jacobian rows,
// contact records, the tableau when it does not fit in LDS).
int32_t plan_wide(Ctx& c) {
  const HostModel& m = c.m;
  const MkhProblemDesc& d = c.d;
  WidePlan& wp = c.pl.wide;
  WideProblem& W = wp.W;
  memset(&W, 0, sizeof W);
  const int nv = m.nv, nb = m.nbody, nj = m.njnt;
  W.nq = m.nq; W.nv = nv; W.nbody = nb; W.njnt = nj; W.robot_root = 1;
  W.n_frame = d.n_frame_tasks; W.n_posture = d.n_posture_tasks; W.n_com = d.n_com_tasks;
  W.n_cfg = d.n_configuration_limits; W.n_vel = d.n_velocity_limits; W.n_pairs = (int)c.pl.pairs.size();
  W.n_dense_tasks = d.n_dense_tasks; W.n_dense_rows = (int)c.pl.dcost.size(); W.n_dense_limit_rows = d.n_dense_limit_rows;
  W.dense_box = d.dense_limit_box ? 1 : 0;
  W.nlevels = m.nlevels;
  W.chain_words = m.chain_words;
  // ---- tasks and limits, one value per dof
  dof_tables(c, nv, true, wp.pcost, wp.clo, wp.chi, wp.vlim);
  for (int t = 0; t < W.n_posture; ++t) { W.posture_gain[t] = d.posture_tasks[t].gain; W.posture_lm[t] = d.posture_tasks[t].lm_damping; }
  int jrows = 0;
  for (const auto& f : c.pl.ft) jrows += __builtin_popcount(f.rowmask);      // (FrameTaskDev::jrow0 counts the same way)
  for (int t = 0; t < W.n_com; ++t) {
    W.com_rowmask[t] = 0;
    for (int k = 0; k < 3; ++k) { W.com_cost[t][k] = d.com_tasks[t].cost[k]; if (d.com_tasks[t].cost[k] != 0.0) W.com_rowmask[t] |= 1 << k; }
    W.com_gain[t] = d.com_tasks[t].gain; W.com_lm[t] = d.com_tasks[t].lm_damping;
    W.com_jrow0[t] = jrows; jrows += __builtin_popcount(W.com_rowmask[t]);
  }
  W.n_jrows = jrows;
  // rows of the (e, J) tap layout — the same order plan_task_rows counts for the wavefront kernels (DeviceProblem::n_rows_tap)
  {
    int row = 6 * W.n_frame;
    for (int t = 0; t < W.n_posture; ++t) { W.posture_row0[t] = row; row += nv; }
    for (int t = 0; t < W.n_com; ++t) { W.com_row0[t] = row; row += 3; }
    W.dense_tap_row0 = row;
    for (int t = 0; t < W.n_dense_tasks; ++t) row += d.dense_tasks[t].k;
    W.n_rows_tap = row;
  }
  for (int t = 0, r0 = 0; t < W.n_dense_tasks; ++t) {
    W.dense_row0[t] = r0; W.dense_k[t] = d.dense_tasks[t].k; W.dense_lm[t] = d.dense_tasks[t].lm_damping; r0 += d.dense_tasks[t].k;
  }
  for (int t = 0; t < W.n_cfg; ++t) W.cfg_gain[t] = d.configuration_limits[t].gain;
  // ---- LDS layout and the per-workgroup slice of device memory
  const int rows_max = W.n_pairs + W.n_dense_limit_rows;
  W.max_rows = rows_max < kWideMaxRows ? rows_max : kWideMaxRows;
  const int Ncap = nv + W.max_rows, R_all = W.n_jrows + W.n_dense_rows;
  auto ev = [](int x) { return (x + 1) & ~1; };
  // more than a wavefront of pairs: bounding-sphere cull in front of the distance routines (wide_contacts; the candidate list —
  // 16-bit pair indices — lives in the three QP vectors behind o_rown, which are dead until the tableau is built)
  wp.use_cull = W.n_pairs > kWave && W.n_pairs < 65536 && W.n_pairs <= 12 * ev(Ncap) && c.pl.culls.size() == c.pl.pairs.size() &&
                !(c.diag & MKH_DIAG_NO_PAIR_CULL);
  int o = 0;
  W.o_q = o; o += ev(W.nq);
  W.o_X = o; o += ev(7 * nb);
  W.o_jnt = o; o += ev(6 * (nj > 0 ? nj : 1));
  W.o_dof = o; o += 10 * nv;
  W.o_task = o; o += 64 * (W.n_frame > 0 ? W.n_frame : 1);
  W.o_com = o; o += W.n_com > 0 ? 4 * nb : 0;
  W.o_we = o; o += ev(R_all > 0 ? R_all : 1);
  W.o_c = o; o += ev(nv);
  W.o_hd = o; o += ev(nv);
  W.o_z = o; o += ev(Ncap); W.o_w = o; o += ev(Ncap); W.o_lo = o; o += ev(nv); W.o_hi = o; o += ev(nv);
  W.o_rown = o; o += ev(Ncap); W.o_ref = o; o += ev(Ncap); W.o_col = o; o += ev(Ncap);
  W.o_red = o; o += kWideThreads + kWideThreads / 2;
  W.o_state = o; o += ev((Ncap + 1) / 2);
  W.o_cws = o; o += c.pl.sel.convex_pairs ? 4 * kConvexWsDoubles : 0;
  const int lds_cap = (160 * 1024 - 2048) / 8;                              // doubles of LDS one workgroup may take
  // staging vectors of the block pivots (wide_kernel.h wide_rank4): over the poses / joint axes when they fit, else appended — unless
  // that would push the tableau out of LDS or cost the second resident workgroup
  W.blk_stride = ev(Ncap);
  W.o_blk = -1;
  if (8 * W.blk_stride <= W.o_dof - W.o_X) W.o_blk = W.o_X;
  else {
    const long long with = (long long)o + 8 * W.blk_stride, t = (long long)Ncap * Ncap;
    const bool keeps_t = (with + t <= lds_cap) == ((long long)o + t <= lds_cap);
    const long long tot0 = (long long)o + ((long long)o + t <= lds_cap ? t : 0), tot1 = with + (with + t <= lds_cap ? t : 0);
    const bool keeps_two = (tot1 * 8 <= 80 * 1024) == (tot0 * 8 <= 80 * 1024);
    if (with <= lds_cap && keeps_t && keeps_two) { W.o_blk = o; o += 8 * W.blk_stride; }
  }
  W.tableau_in_lds = (long long)o + (long long)Ncap * Ncap <= lds_cap ? 1 : 0;
  // the dense Goldfarb–Idnani fallback's factors (2·nv² + 2·nv + 8 doubles) in LDS when that costs neither the tableau's place nor
  // the second resident workgroup
  const long long gi_sz = rows_max > 0 ? 2ll * nv * (nv | 1) + 4ll * (nv + 2) : 0;
  const int two_wg = 80 * 1024 / 8;
  W.o_gi = o; W.gi_in_lds = 0;
  if (gi_sz > 0 && (long long)o + gi_sz + (long long)(nv + 8) * (nv + 8) <= two_wg) { W.gi_in_lds = 1; o += (int)gi_sz; }
  W.o_T = o;
  if (W.tableau_in_lds) { W.t_lds_doubles = Ncap * Ncap; o += Ncap * Ncap; }
  else {
    // the largest instance does not fit: reserve what keeps two workgroups resident (or, failing that, what is left) for the
    // instances that do — most have far fewer rows in range than the limit lists pairs
    long long room = (long long)two_wg - o;
    if (room < (long long)(nv + 8) * (nv + 8)) room = (long long)lds_cap - o;
    W.t_lds_doubles = room > 0 ? (int)room : 0;
    o += W.t_lds_doubles;
  }
  W.lds_doubles = o;
  if (o > lds_cap)
    return c.fail(MKH_E_LIMIT, "model too large for the workgroup-per-problem kernel: %d KB of LDS per problem, 158 KB available (per problem "
                  "≈ 8·(nq + 7·nbody + 6·njnt + 14·nv + 5.5·(nv + rows) + 64·frame tasks) bytes: a serial chain fits up to ≈ 550 dofs)", o / 128);
  long long w = 0;
  W.ws_jw = w; w += (long long)(R_all > 0 ? R_all : 1) * nv;
  W.ws_rec = w; w += (long long)(W.n_pairs > 0 ? W.n_pairs : 1) * 10;
  W.ws_rowpair = w; w += ev((W.max_rows + 2) / 2);
  W.ws_rank = w; w += ev((W.n_pairs + 2) / 2);
  W.ws_T = w; w += W.tableau_in_lds ? 0 : (long long)Ncap * Ncap;
  W.ws_gi = w; w += rows_max > 0 ? 2ll * nv * (nv | 1) + 4ll * (nv + 2) : 0;
  W.ws_stride = (w + 15) & ~15ll;
  const int per_cu = (160 * 1024) / (o * 8) < 2 ? ((160 * 1024) / (o * 8) < 1 ? 1 : (160 * 1024) / (o * 8)) : 2;
  int grid = c.num_cus * per_cu;
  if (grid > c.max_batch) grid = c.max_batch;
  while (grid > 1 && (long long)grid * W.ws_stride * 8 > (1ll << 30)) grid /= 2;      // (≤ 1 GB of slices)
  wp.ws_doubles = (long long)grid * W.ws_stride;
  c.pl.sel.wide_grid = grid; c.pl.sel.wide_lds = o * 8;
  uint32_t cap = 256;
  while (cap < (uint32_t)c.max_batch) cap *= 2;
  wp.redo_cap = cap;
  W.redo_cap = cap; W.redo_pad = 0;
  wp.built = true;
  return MKH_OK;
}

// ---- 13. The two-kernel split of general convex pairs (convex_pre.hip): per convex pair the chains root → body of its two geoms
// (the buffer of pre-evaluated contacts the analytic build reads is the upload's).  It uses the plain model arrays of the twin above.
void plan_convex_split(Ctx& c) {
  ProblemPlan& pl = c.pl;
  if (!pl.wide.built || pl.n_cv == 0 || c.sw.no_convex_split) { pl.n_cv = 0; return; }   // (A/B: the in-kernel routine, round 4's path)
  pl.cv_adr.push_back(0);
  for (size_t k = 0; k < pl.pairs.size(); ++k) {
    if (pl.pairs[k].cv_slot < 0) continue;
    pl.cv_pair.push_back((int32_t)k);
    for (int body : {pl.pairs[k].body1, pl.pairs[k].body2}) {
      std::vector<int32_t> up;
      for (int b = body; b > 0; b = c.m.body_parentid[b]) up.push_back(b);
      pl.cv_chain.insert(pl.cv_chain.end(), up.rbegin(), up.rend());
      pl.cv_adr.push_back((int32_t)pl.cv_chain.size());
    }
  }
  pl.dev.n_cv = pl.n_cv;
}

}  // namespace

int32_t plan_problem(const HostModel& m, const MkhProblemDesc& d, int diag, int max_batch, int num_cus, const PlanSwitches& sw,
                     ProblemPlan& plan, std::string& err) {
  Ctx c{m, d, diag, max_batch, num_cus, sw, plan, Fail{err}};
  if (const int32_t rc = validate(c)) return rc;
  plan_task_rows(c);
  plan_box_limits(c);
  plan_pairs(c);
  if (m.big) {
    // beyond one wavefront: the workgroup-per-problem kernel takes every call of this problem (wide_kernel.h)
    if (const int32_t rc = plan_wide(c)) return rc;
    plan.sel.wide_only = true;
    plan.n_cv = 0;
    plan.dev.n_rows_tap = plan.wide.W.n_rows_tap;        // (what mkh_problem_num_task_rows reports; the wavefront descriptor is not built)
    return MKH_OK;
  }
  if (const int32_t rc = plan_tableau(c)) return rc;
  if (const int32_t rc = plan_direct_layouts(c)) return rc;
  plan_direct_pairs(c);
  plan_wood(c);
  plan_wood_rows(c);
  plan_lane(c);
  plan_tight_rows(c);
  // More rows can be active at once than the 64 − nv the wavefront kernels hold (the reference stacks them all:
  // mink/solve_ik.py:25-40): the instances a launch flags MKH_ST_ROW_OVERFLOW are solved again by the workgroup-per-problem
  // kernel with every row (launch(): the redo launch behind plain solves)
  // (round 5: EVERY problem with half-space rows gets this twin — its dense Goldfarb–Idnani iteration also re-solves the instances
  //  whose active rows are almost dependent, wherever they occur; MKH_DIAG_NO_WIDE_REDO: what the wavefront kernel alone leaves flagged)
  if (!(diag & MKH_DIAG_NO_WIDE_REDO) && plan.dev.n_pairs + plan.dev.n_dense_limit_rows > 0)
    if (const int32_t rc = plan_wide(c)) return rc;
  plan_convex_split(c);
  return MKH_OK;
}

}  // namespace mkh
