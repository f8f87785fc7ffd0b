// Host-only driver of mink_amd/csrc/problem_plan.hip for tests/test_problem_plan_cpu.py: synthetic models and descriptors that
// put every fixed-size table of the device descriptor at its edge, planned without a device and printed as one JSON object per
// line — among them lists of 2 to 4 limits of each kind (and 5: refused) whose terms have their own gain, bounds and index subset,
// printed with every copy of the per-dof tables the plan makes of them.  Built with the host sanitizers by the test and run as a
// child process.
//
// With a file name as its argument the program also plans the models that file describes — the large models of tests/wide_cases.py,
// taken from the same MJCF text the device tests load: one line each,
//   name  spheres(0/1)  n  (parent kind)·n  n_tasks  body·n_tasks  n_com  n_pairs  (geom geom)·n_pairs
// planned once (case `wide`: six-row frame tasks on the given bodies, a posture task, ConfigurationLimit, VelocityLimit, the pairs
// in one CollisionAvoidanceLimit) and printed with the chain bit table of every body.
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../mink_amd/csrc/problem_plan.h"

using namespace mkh;

namespace {

enum Kind { FIXED = 0, HINGE = 1, HINGE2 = 2, BALL = 3, FREE = 4, SLIDE = 5 };
struct BodySpec { int parent; int kind; };

// A flat model and the arrays it points to.
struct Model {
  std::string name;
  std::vector<int32_t> body_parentid, body_rootid, body_jntnum, body_jntadr, body_dofnum, body_dofadr;
  std::vector<double> body_pos, body_quat, body_ipos, body_mass, body_subtreemass;
  std::vector<int32_t> jnt_type, jnt_qposadr, jnt_dofadr, jnt_bodyid, jnt_limited;
  std::vector<double> jnt_pos, jnt_axis, jnt_range, qpos0;
  std::vector<int32_t> dof_bodyid, dof_jntid, dof_parentid, site_bodyid, geom_bodyid, geom_type;
  std::vector<double> site_pos, site_quat, geom_size, geom_pos, geom_quat;
  std::vector<int> leaves;
  int cyl_geom = 0, box_geom = 0;
  MkhFlatModel flat{};
};

void make_model(Model& M, const std::string& name, const std::vector<BodySpec>& spec, bool spheres = false) {
  M.name = name;
  const int nb = (int)spec.size() + 1;
  M.body_parentid.assign(nb, 0); M.body_rootid.assign(nb, 0); M.body_jntnum.assign(nb, 0); M.body_jntadr.assign(nb, -1);
  M.body_dofnum.assign(nb, 0); M.body_dofadr.assign(nb, -1);
  M.body_pos.assign(3 * nb, 0.0); M.body_quat.assign(4 * nb, 0.0); M.body_ipos.assign(3 * nb, 0.0);
  M.body_mass.assign(nb, 1.0); M.body_subtreemass.assign(nb, 0.0);
  M.body_mass[0] = 0.0;
  std::vector<int> last_dof(nb, -1), has_child(nb, 0);
  int nq = 0, nv = 0;
  for (int b = 0; b < nb; ++b) M.body_quat[4 * b] = 1.0;
  for (int b = 1; b < nb; ++b) {
    const BodySpec& s = spec[b - 1];
    M.body_parentid[b] = s.parent;
    has_child[s.parent] = 1;
    M.body_rootid[b] = s.parent == 0 ? b : M.body_rootid[s.parent];
    M.body_pos[3 * b + 2] = 0.1;
    last_dof[b] = last_dof[s.parent];
    const int nj = s.kind == FIXED ? 0 : (s.kind == HINGE2 ? 2 : 1);
    if (nj) { M.body_jntadr[b] = (int)M.jnt_type.size(); M.body_dofadr[b] = nv; }
    M.body_jntnum[b] = nj;
    for (int i = 0; i < nj; ++i) {
      const int jt = s.kind == FREE ? JNT_FREE : (s.kind == BALL ? JNT_BALL : (s.kind == SLIDE ? JNT_SLIDE : JNT_HINGE));
      const int ndof = jt == JNT_FREE ? 6 : (jt == JNT_BALL ? 3 : 1), nqj = jt == JNT_FREE ? 7 : (jt == JNT_BALL ? 4 : 1);
      const int j = (int)M.jnt_type.size();
      M.jnt_type.push_back(jt); M.jnt_qposadr.push_back(nq); M.jnt_dofadr.push_back(nv); M.jnt_bodyid.push_back(b);
      M.jnt_limited.push_back(jt == JNT_HINGE || jt == JNT_SLIDE ? 1 : 0);
      for (int k = 0; k < 3; ++k) { M.jnt_pos.push_back(0.0); M.jnt_axis.push_back(k == (j % 3) ? 1.0 : 0.0); }
      M.jnt_range.push_back(-2.0); M.jnt_range.push_back(2.0);
      for (int k = 0; k < nqj; ++k) M.qpos0.push_back((jt == JNT_FREE && k == 3) || (jt == JNT_BALL && k == 0) ? 1.0 : 0.0);
      for (int k = 0; k < ndof; ++k) {
        M.dof_bodyid.push_back(b); M.dof_jntid.push_back(j); M.dof_parentid.push_back(last_dof[b]);
        last_dof[b] = nv++;
      }
      nq += nqj;
      M.body_dofnum[b] += ndof;
    }
  }
  for (int b = nb - 1; b >= 1; --b) {
    M.body_subtreemass[b] += M.body_mass[b];
    M.body_subtreemass[M.body_parentid[b]] += M.body_subtreemass[b];
    if (!has_child[b]) M.leaves.insert(M.leaves.begin(), b);
  }
  // one capsule per moving body, then a cylinder on the last body and a box on the first; one site on the last body
  for (int b = 1; b < nb; ++b) { M.geom_bodyid.push_back(b); M.geom_type.push_back(spheres ? PLAN_GEOM_SPHERE : PLAN_GEOM_CAPSULE); }
  M.cyl_geom = (int)M.geom_type.size(); M.geom_bodyid.push_back(nb - 1); M.geom_type.push_back(PLAN_GEOM_CYLINDER);
  M.box_geom = (int)M.geom_type.size(); M.geom_bodyid.push_back(1); M.geom_type.push_back(PLAN_GEOM_BOX);
  const int ng = (int)M.geom_type.size();
  M.geom_size.assign(3 * ng, 0.03); M.geom_pos.assign(3 * ng, 0.0); M.geom_quat.assign(4 * ng, 0.0);
  for (int g = 0; g < ng; ++g) M.geom_quat[4 * g] = 1.0;
  M.site_bodyid = {nb - 1}; M.site_pos = {0.0, 0.0, 0.05}; M.site_quat = {1.0, 0.0, 0.0, 0.0};
  MkhFlatModel& h = M.flat;
  h.nq = nq; h.nv = nv; h.nbody = nb; h.njnt = (int)M.jnt_type.size(); h.ngeom = ng; h.nsite = 1;
  h.body_parentid = M.body_parentid.data(); h.body_rootid = M.body_rootid.data(); h.body_jntnum = M.body_jntnum.data();
  h.body_jntadr = M.body_jntadr.data(); h.body_dofnum = M.body_dofnum.data(); h.body_dofadr = M.body_dofadr.data();
  h.body_pos = M.body_pos.data(); h.body_quat = M.body_quat.data(); h.body_ipos = M.body_ipos.data();
  h.body_mass = M.body_mass.data(); h.body_subtreemass = M.body_subtreemass.data();
  h.jnt_type = M.jnt_type.data(); h.jnt_qposadr = M.jnt_qposadr.data(); h.jnt_dofadr = M.jnt_dofadr.data();
  h.jnt_bodyid = M.jnt_bodyid.data(); h.jnt_limited = M.jnt_limited.data();
  h.jnt_pos = M.jnt_pos.data(); h.jnt_axis = M.jnt_axis.data(); h.jnt_range = M.jnt_range.data(); h.qpos0 = M.qpos0.data();
  h.dof_bodyid = M.dof_bodyid.data(); h.dof_jntid = M.dof_jntid.data(); h.dof_parentid = M.dof_parentid.data();
  h.site_bodyid = M.site_bodyid.data(); h.site_pos = M.site_pos.data(); h.site_quat = M.site_quat.data();
  h.geom_bodyid = M.geom_bodyid.data(); h.geom_type = M.geom_type.data();
  h.geom_size = M.geom_size.data(); h.geom_pos = M.geom_pos.data(); h.geom_quat = M.geom_quat.data();
}

std::vector<BodySpec> chain(int nbodies, int first_kind = HINGE) {
  std::vector<BodySpec> s;
  for (int i = 0; i < nbodies; ++i) s.push_back({i, i == 0 ? first_kind : HINGE});
  return s;
}
// a free root and limbs of the given numbers of hinges, each a serial chain off the root
std::vector<BodySpec> tree(const std::vector<int>& limbs) {
  std::vector<BodySpec> s{{0, FREE}};
  for (int n : limbs)
    for (int i = 0; i < n; ++i) s.push_back({i == 0 ? 1 : (int)s.size(), HINGE});
  return s;
}

// One descriptor: the frame tasks as (body, root body or −1, active rows: the first `rows` costs are 1), then the counts of everything else.
struct TaskSpec { int body, root, rows; };
enum Bad { BAD_NONE = 0, BAD_DOF_RANGE, BAD_COST, BAD_FRAME_ID, BAD_FREE_LIMIT, BAD_BALL_SLOTS };
struct Case {
  std::string name;
  std::vector<TaskSpec> tasks;
  int n_com = 0, n_pairs = 0, n_boxpairs = 0;
  bool cylbox = false, dense = false;
  int diag = 0, bad = BAD_NONE;
  std::vector<int32_t> pair_list;                 // explicit geom pairs (a, b, a, b, …) in front of the counted ones
  bool print_chain = false;
  // lists of limits (n_cfg >= 0): that many ConfigurationLimits / VelocityLimits, each with its own gain, bounds and index subset,
  // two PostureTasks, and the capsule pairs split over n_col CollisionAvoidanceLimits with their own parameters
  int n_cfg = -1, n_vel = 1, n_col = 1;
  Case& lists(int c, int v, int col = 1) { n_cfg = c; n_vel = v; n_col = col; return *this; }
};

// One term of a list of limits: the arrays a descriptor points to.
struct BoxTerm {
  double gain = 0.0;
  std::vector<int32_t> idx;
  std::vector<double> lower, upper, limit;
};

void put(const char* key, long long v, bool comma = true) { printf("\"%s\":%lld%s", key, v, comma ? "," : ""); }
template <class T>
void put_arr(const char* key, const T* a, size_t n, bool comma = true) {
  printf("\"%s\":[", key);
  for (size_t i = 0; i < n; ++i) printf("%s%lld", i ? "," : "", (long long)a[i]);
  printf("]%s", comma ? "," : "");
}
void put_u64(const char* key, const uint64_t* a, size_t n) {       // (as strings: JSON numbers stop at 2^53)
  printf("\"%s\":[", key);
  for (size_t i = 0; i < n; ++i) printf("%s\"%llu\"", i ? "," : "", (unsigned long long)a[i]);
  printf("],");
}
// doubles as %.17g (read back exactly); the infinities as the tokens Python's json module reads
void put_dbl(const char* key, const double* a, size_t n, bool comma = true) {
  printf("\"%s\":[", key);
  for (size_t i = 0; i < n; ++i) {
    if (a[i] == a[i] && (a[i] - a[i]) != 0.0) printf("%s%sInfinity", i ? "," : "", a[i] < 0 ? "-" : "");
    else printf("%s%.17g", i ? "," : "", a[i]);
  }
  printf("]%s", comma ? "," : "");
}
// the box and posture tables of a lane descriptor, [term][MD] flattened
template <int ML, int MD>
void put_lane(const char* key, const LaneProblemT<ML, MD>& L) {
  printf("\"%s\":{", key);
  put("md", MD); put("n_posture", L.n_posture); put("n_cfg", L.n_cfg); put("n_vel", L.n_vel);
  put_dbl("cfg_gain", L.cfg_gain, kMaxBoxTerms); put_dbl("cfg_lower", &L.cfg_lower[0][0], (size_t)kMaxBoxTerms * MD);
  put_dbl("cfg_upper", &L.cfg_upper[0][0], (size_t)kMaxBoxTerms * MD); put_dbl("vel_limit", &L.vel_limit[0][0], (size_t)kMaxBoxTerms * MD);
  put_dbl("posture_cost", &L.posture_cost[0][0], (size_t)kMaxPostureTasks * MD);
  put_dbl("posture_gain", L.posture_gain, kMaxPostureTasks); put_dbl("posture_lm", L.posture_lm, kMaxPostureTasks, false);
  printf("},");
}
void put_str(const char* key, const std::string& s) {
  printf("\"%s\":\"", key);
  for (char ch : s) { if (ch == '"' || ch == '\\') putchar('\\'); putchar(ch); }
  printf("\",");
}
int total8(const DeviceProblem& D, int nt, int nr, int feat, bool w3) { return 8 * build_lds_layout(D, nt, nr, feat, w3).total; }

void put_dev(const char* key, const DeviceProblem& P) {
  printf("\"%s\":{", key);
  put("nv", P.nv); put("n_frame", P.n_frame); put("n_com", P.n_com); put("n_pairs", P.n_pairs); put("max_rows", P.max_rows);
  put("n_jrows", P.n_jrows); put("n_rows_tap", P.n_rows_tap); put("nt", P.nt); put("n_hsel", P.n_hsel); put("n_cv", P.n_cv);
  put("prefetch", P.prefetch); put("prefetch_w3", P.prefetch_w3); put("prefetch_w3w", P.prefetch_w3w); put("prefetch_wc", P.prefetch_wc);
  put("wood_compact", P.wood_compact); put("wood_refine", P.wood_refine);
  put("wood_rpc", P.wood_rpc); put("wood_trip", P.wood_trip); put("wood_jrhs", P.wood_jrhs);
  put_arr("wood_col", P.wood_col, 64); put_arr("wood_row0", P.wood_row0, 64); put_u64("wood_mask", P.wood_mask, 64);
  put_arr("wood_list", &P.wood_list[0][0], 256);
  put("n_jpairs", P.n_jpairs); put_arr("jpair_task", P.jpair_task, 256); put_arr("jpair_dof", P.jpair_dof, 256);
  put_arr("mu_src", P.mu_src, 64);
  put("n_dpairs", P.n_dpairs); put_arr("dpair_task", P.dpair_task, 64); put_arr("dpair_dof", P.dpair_dof, 64, false);
  printf("},");
}

void run_case(const Model& M, const HostModel& hm, const Case& cs) {
  const int nv = hm.nv, nq = hm.nq, nb = hm.nbody;
  std::vector<MkhFrameTaskDesc> ft;
  for (const TaskSpec& t : cs.tasks) {
    MkhFrameTaskDesc f{};
    f.frame_type = MKH_FRAME_BODY; f.frame_id = t.body;
    for (int k = 0; k < 6; ++k) f.cost[k] = k < t.rows ? 1.0 : 0.0;      // (5 rows: one orientation cost 0; 3: position only)
    f.gain = 1.0; f.lm_damping = 1e-3;
    f.root_type = t.root >= 0 ? MKH_FRAME_BODY : -1; f.root_id = t.root >= 0 ? t.root : 0;
    ft.push_back(f);
  }
  if (cs.bad == BAD_COST) ft.at(0).cost[1] = -1.0;
  if (cs.bad == BAD_FRAME_ID) ft.at(0).frame_id = nb;
  std::vector<double> pcost(nv, 0.1), lower(nq, -1.0), upper(nq, 1.0), vmax(nv, 3.0);
  const bool lists = cs.n_cfg >= 0;
  std::vector<double> pcost1(nv);
  for (int dd = 0; dd < nv; ++dd) pcost1[dd] = 0.25 + 0.015625 * dd;
  MkhPostureTaskDesc pts[2] = {{pcost.data(), 1.0, 0.0}, {pcost1.data(), 0.5, 0.125}};
  MkhComTaskDesc ct{{1.0, 1.0, 0.0}, 1.0, 0.0};
  std::vector<int32_t> lim_dofs, all_dofs;
  for (int dd = 0; dd < nv; ++dd) {
    all_dofs.push_back(dd);
    if (hm.jnt_type[hm.dof_jntid[dd]] != JNT_FREE) lim_dofs.push_back(dd);
  }
  if (cs.bad == BAD_DOF_RANGE) lim_dofs.push_back(nv);
  if (cs.bad == BAD_FREE_LIMIT) lim_dofs.push_back(0);
  if (cs.bad == BAD_BALL_SLOTS)                   // a ball joint's four qpos slots of `upper` holding a quaternion of their own
    for (int dd = 0; dd < nv; ++dd)
      if (hm.jnt_type[hm.dof_jntid[dd]] == JNT_BALL) upper[hm.jnt_qposadr[hm.dof_jntid[dd]] + 2] = 0.5;
  // the terms of a list.  Index subsets over the limited dofs L: configuration term 0 the even positions of L, term 1 the odd ones
  // (disjoint: a dof of term 1 is in no term before it), term 2 all of L backwards, term 3 and 4 every third; velocity term 0 the
  // first half, term 1 the second half and its last dof named three more times (four in all: a smaller limit between two larger ones), term 2 all,
  // term 3 and 4 the first dof of L alone.  Bounds are indexed by qpos address, limits by position in the term.
  std::vector<BoxTerm> cterm(lists ? cs.n_cfg : 0), vterm(lists ? cs.n_vel : 0);
  const int nl = (int)lim_dofs.size();
  for (int t = 0; t < (int)cterm.size(); ++t) {
    BoxTerm& b = cterm[t];
    const double gains[5] = {0.95, 0.5, 1.0, 0.25, 0.75};
    b.gain = gains[t];
    for (int k = 0; k < nl; ++k)
      if (t == 0 ? k % 2 == 0 : (t == 1 ? k % 2 == 1 : (t == 2 ? true : k % 3 == 0))) b.idx.push_back(lim_dofs[t == 2 ? nl - 1 - k : k]);
    b.lower.resize(nq); b.upper.resize(nq);
    for (int a = 0; a < nq; ++a) { b.lower[a] = -1.0 - 0.125 * t - 0.0078125 * a; b.upper[a] = 0.5 + 0.25 * t + 0.00390625 * a; }
    for (int dd = 0; dd < nv; ++dd)                 // (a ball joint: one value over its four slots, or the descriptor is refused)
      if (hm.jnt_type[hm.dof_jntid[dd]] == JNT_BALL) {
        const int qa = hm.jnt_qposadr[hm.dof_jntid[dd]];
        for (int k = 1; k < 4; ++k) { b.lower[qa + k] = b.lower[qa]; b.upper[qa + k] = b.upper[qa]; }
      }
  }
  for (int t = 0; t < (int)vterm.size(); ++t) {
    BoxTerm& b = vterm[t];
    for (int k = 0; k < nl; ++k)
      if (t == 0 ? k < nl / 2 : (t == 1 ? k >= nl / 2 : (t == 2 ? true : k == 0))) b.idx.push_back(lim_dofs[k]);
    for (size_t k = 0; k < b.idx.size(); ++k) b.limit.push_back(2.0 + 0.5 * t + 0.03125 * (double)k);
    if (t == 1) for (double x : {1.75, 0.375, 1.5}) { b.idx.push_back(lim_dofs[nl - 1]); b.limit.push_back(x); }
  }
  std::vector<MkhConfigurationLimitDesc> cls;
  std::vector<MkhVelocityLimitDesc> vls;
  for (BoxTerm& b : cterm) cls.push_back({b.gain, b.lower.data(), b.upper.data(), (int32_t)b.idx.size(), b.idx.data()});
  for (BoxTerm& b : vterm) vls.push_back({(int32_t)b.idx.size(), b.idx.data(), b.limit.data()});
  if (!lists) {
    cls.push_back({0.5, lower.data(), upper.data(), (int32_t)lim_dofs.size(), lim_dofs.data()});
    vls.push_back({(int32_t)all_dofs.size(), all_dofs.data(), vmax.data()});
  }
  // capsule pairs: the capsule of the last body against those of the first ones (cycling), then the cylinder against the box
  std::vector<int32_t> gp = cs.pair_list;
  for (int k = 0; k < cs.n_pairs; ++k) { gp.push_back(nb - 2); gp.push_back(k % (nb - 2)); }
  for (int k = 0; k < cs.n_boxpairs; ++k) { gp.push_back(nb - 2 - k % (nb - 2)); gp.push_back(M.box_geom); }   // capsules against the box
  if (cs.cylbox) { gp.push_back(M.cyl_geom); gp.push_back(M.box_geom); }
  // two CollisionAvoidanceLimits: the second takes the pairs from the last one of the first onwards (one geom pair is in both)
  // and has its own four parameters
  std::vector<int32_t> gp1;
  if (cs.n_col == 2 && gp.size() >= 4) gp1.assign(gp.begin() + ((gp.size() / 4) * 2 - 2), gp.end()), gp.resize((gp.size() / 4) * 2);
  std::vector<MkhCollisionLimitDesc> cols;
  if (!gp.empty()) cols.push_back({(int32_t)gp.size() / 2, gp.data(), 0.85, 0.005, 0.01, 0.0});
  if (!gp1.empty()) cols.push_back({(int32_t)gp1.size() / 2, gp1.data(), 0.5, 0.02, 0.05, 1e-3});
  const double dense_cost[3] = {1.0, 0.5, 0.25};
  MkhDenseTaskDesc dt{3, dense_cost, 1.0, 0.0};
  MkhProblemDesc d{};
  d.n_frame_tasks = (int32_t)ft.size(); d.frame_tasks = ft.data();
  d.n_posture_tasks = lists ? 2 : 1; d.posture_tasks = pts;
  d.n_com_tasks = cs.n_com; d.com_tasks = &ct;
  d.n_configuration_limits = (int32_t)cls.size(); d.configuration_limits = cls.data();
  d.n_velocity_limits = (int32_t)vls.size(); d.velocity_limits = vls.data();
  d.n_collision_limits = (int32_t)cols.size(); d.collision_limits = cols.data();
  d.n_dense_tasks = cs.dense ? 1 : 0; d.dense_tasks = &dt;

  ProblemPlan plan;
  std::string err;
  const int32_t rc = plan_problem(hm, d, cs.diag, 64, 256, PlanSwitches{}, plan, err);

  printf("{");
  put_str("model", M.name); put_str("case", cs.name);
  put("nv", nv); put("nq", nq); put("nbody", nb); put("njnt", hm.njnt); put("big", hm.big);
  if (cs.print_chain) { put("model_chain_words", hm.chain_words); put_u64("chain", hm.chain.data(), hm.chain.size()); }
  put_arr("body_parentid", hm.body_parentid.data(), nb); put_arr("body_dofadr", hm.body_dofadr.data(), nb);
  put_arr("body_dofnum", hm.body_dofnum.data(), nb);
  printf("\"tasks\":[");
  for (size_t t = 0; t < ft.size(); ++t) {
    printf("%s{", t ? "," : "");
    put("body", cs.tasks[t].body); put("root", cs.tasks[t].root);
    printf("\"cost\":[");
    for (int k = 0; k < 6; ++k) printf("%s%g", k ? "," : "", ft[t].cost[k]);
    printf("]}");
  }
  printf("],");
  put("n_com", cs.n_com); put("com_rows", cs.n_com ? 2 : 0); put("n_pairs_in", (long long)(gp.size() + gp1.size()) / 2); put("cylbox", cs.cylbox);
  put("n_posture", d.n_posture_tasks); put("lists", lists);
  if (lists) {
    // the descriptor as handed over, and per dof what indexes it: the joint's qpos address and whether the joint is a free one
    std::vector<int32_t> qa(nv), fr(nv);
    for (int dd = 0; dd < nv; ++dd) { qa[dd] = hm.jnt_qposadr[hm.dof_jntid[dd]]; fr[dd] = hm.jnt_type[hm.dof_jntid[dd]] == JNT_FREE; }
    put_arr("dof_qposadr", qa.data(), nv); put_arr("dof_free", fr.data(), nv);
    printf("\"desc\":{\"cfg\":[");
    for (size_t t = 0; t < cterm.size(); ++t) {
      printf("%s{", t ? "," : "");
      put_dbl("gain", &cterm[t].gain, 1); put_arr("indices", cterm[t].idx.data(), cterm[t].idx.size());
      put_dbl("lower", cterm[t].lower.data(), nq); put_dbl("upper", cterm[t].upper.data(), nq, false);
      printf("}");
    }
    printf("],\"vel\":[");
    for (size_t t = 0; t < vterm.size(); ++t) {
      printf("%s{", t ? "," : "");
      put_arr("indices", vterm[t].idx.data(), vterm[t].idx.size()); put_dbl("limit", vterm[t].limit.data(), vterm[t].limit.size(), false);
      printf("}");
    }
    printf("],\"col\":[");
    for (size_t t = 0; t < cols.size(); ++t) {
      const double par[4] = {cols[t].gain, cols[t].minimum_distance_from_collisions, cols[t].collision_detection_distance, cols[t].bound_relaxation};
      printf("%s{", t ? "," : "");
      put_arr("pairs", cols[t].geom_id_pairs, 2 * (size_t)cols[t].n_pairs); put_dbl("par", par, 4, false);
      printf("}");
    }
    printf("],\"post\":[");
    for (int t = 0; t < d.n_posture_tasks; ++t) {
      const double gl[2] = {pts[t].gain, pts[t].lm_damping};
      printf("%s{", t ? "," : "");
      put_dbl("cost", pts[t].cost, nv); put_dbl("gain_lm", gl, 2, false);
      printf("}");
    }
    printf("]},");
  }
  put("dense", cs.dense); put("diag", cs.diag); put("rc", rc); put_str("err", err);
  if (rc == MKH_OK) {
    const ProblemSelect& S = plan.sel;
    const DeviceProblem& P = plan.dev;
    printf("\"sel\":{");
    put("nt", S.nt); put("nt_full", S.nt_full); put("lds_bytes", S.lds_bytes); put("lds_bytes_full", S.lds_bytes_full);
    put("lds_bytes_w3", S.lds_bytes_w3); put("blocks_per_cu", S.blocks_per_cu); put("wide_only", S.wide_only);
    put("wide_grid", S.wide_grid); put("wide_lds", S.wide_lds); put("nt_tight", S.nt_tight); put("lds_tight", S.lds_tight);
    put("has_relative", S.has_relative); put("simple_pairs", S.simple_pairs); put("convex_pairs", S.convex_pairs);
    put("wood_nt", S.wood_nt); put("wood_nr", S.wood_nr); put("wood_lds_bytes", S.wood_lds_bytes);
    put("wood_lds_bytes_w3", S.wood_lds_bytes_w3); put("wood_lds_bytes_w4", S.wood_lds_bytes_w4); put("woodr_tables", S.woodr_tables);
    put("woodr_lds", S.woodr_lds); put("woodr_lds_tight", S.woodr_lds_tight); put("wood_big", S.wood_big);
    put("lane_nv", S.lane_nv); put("lane_lds", S.lane_lds); put("quad_nt", S.quad_nt); put("quad_loop_ok", S.quad_loop_ok);
    put("use_cull", S.use_cull, false);
    printf("},");
    put_dev("dev", P);
    put("tight", plan.tight);
    if (plan.tight) put_dev("dev_tight", plan.dev_tight);
    // 8 × total of the layout statement for the build each reserved figure belongs to (lds_layout.h)
    if (!S.wide_only) {
      const int com_feat = (P.n_com > 0 || S.wood_big) ? (F_WOOD | F_COM) : F_WOOD;
      printf("\"layout\":{");
      put("lds_bytes", total8(P, S.nt, 0, F_COLL, false)); put("lds_bytes_full", total8(P, S.nt_full, 0, F_COLL, false));
      put("lds_bytes_w3", total8(P, S.nt, 0, 0, true));
      put("wood_lds_bytes", S.wood_nr ? total8(P, S.wood_nr, S.wood_nr, F_WOOD, false) : 0);
      put("wood_lds_bytes_w3", S.wood_nr ? total8(P, S.wood_nr, S.wood_nr, com_feat, true) : 0);
      put("wood_lds_bytes_w4", S.wood_nr ? 8 * build_lds_layout_w4p(P, S.wood_nr).total : 0);
      put("woodr_lds", total8(P, 48, 48, F_WOOD | F_COLL, false));
      put("lds_tight", plan.tight ? total8(plan.dev_tight, 48, 0, F_COLL, false) : 0);
      put("woodr_lds_tight", plan.tight ? total8(plan.dev_tight, 48, 48, F_WOOD | F_COLL, false) : 0, false);
      printf("},");
    }
    printf("\"lane\":{");
    put("cls", plan.lane_class); put("nq", S.lane_dims.nq); put("nv", S.lane_dims.nv); put("nlink", S.lane_dims.nlink);
    put("n_frame", S.lane_dims.n_frame); put("qadr_identity", S.lane_dims.qadr_identity, false);
    printf("},\"wide\":{");
    const WideProblem& W = plan.wide.W;
    put("built", plan.wide.built); put("nv", W.nv); put("chain_words", W.chain_words); put("nlevels", W.nlevels);
    put("max_rows", W.max_rows); put("n_jrows", W.n_jrows); put("n_rows_tap", W.n_rows_tap); put("lds_doubles", W.lds_doubles);
    put("tableau_in_lds", W.tableau_in_lds); put("ws_stride", W.ws_stride); put("ws_doubles", plan.wide.ws_doubles);
    put("redo_cap", plan.wide.redo_cap); put("use_cull", plan.wide.use_cull);
    // the staging vectors of the block pivots: over the poses (overlay), behind the QP vectors (appended), or none (absent)
    put("o_X", W.o_X); put("o_blk", W.o_blk); put("blk_stride", W.blk_stride); put("t_lds_doubles", W.t_lds_doubles);
    put("n_frame", W.n_frame); put("n_pairs", W.n_pairs); put("gi_in_lds", W.gi_in_lds);
    put_str("blk", !plan.wide.built ? "" : (W.o_blk < 0 ? "absent" : (W.o_blk == W.o_X ? "overlay" : "appended")));
    put("o_T", W.o_T, false);
    printf("},");
    put("n_cv", plan.n_cv); put_arr("cv_pair", plan.cv_pair.data(), plan.cv_pair.size());
    put_arr("cv_adr", plan.cv_adr.data(), plan.cv_adr.size()); put_arr("cv_chain", plan.cv_chain.data(), plan.cv_chain.size());
    if (lists) {
      // the planned tables: lane tables of the wavefront kernels (stride 64), both lane descriptors, the plain arrays of the
      // workgroup-per-problem kernel (stride nv) and the parameters of every pair
      printf("\"tables\":{");
      put_dbl("cfg_gain", P.cfg_gain, kMaxBoxTerms); put("n_cfg", P.n_cfg); put("n_vel", P.n_vel);
      put_dbl("pcost", plan.pcost.data(), plan.pcost.size()); put_dbl("clo", plan.clo.data(), plan.clo.size());
      put_dbl("chi", plan.chi.data(), plan.chi.size()); put_dbl("vlim", plan.vlim.data(), plan.vlim.size());
      if (plan.lane_class) put_lane("lane2", plan.lane);
      if (plan.lane_class && plan.lane_class != 32) {
        LaneProblem lp1;
        lane_problem_narrow(plan.lane, lp1);
        put_lane("lane1", lp1);
      }
      if (plan.wide.built) {
        const WideProblem& W = plan.wide.W;
        printf("\"wide\":{");
        put("n_cfg", W.n_cfg); put("n_vel", W.n_vel); put("n_posture", W.n_posture); put_dbl("cfg_gain", W.cfg_gain, kMaxBoxTerms);
        put_dbl("pcost", plan.wide.pcost.data(), plan.wide.pcost.size()); put_dbl("clo", plan.wide.clo.data(), plan.wide.clo.size());
        put_dbl("chi", plan.wide.chi.data(), plan.wide.chi.size()); put_dbl("vlim", plan.wide.vlim.data(), plan.wide.vlim.size(), false);
        printf("},");
      }
      std::vector<double> pp;
      for (const CollisionPairDev& cp : plan.pairs) for (double x : {cp.gain, cp.dmin, cp.ddetect, cp.relax}) pp.push_back(x);
      put_dbl("pair_par", pp.data(), pp.size(), false);
      printf("},");
    }
  }
  put("end", 1, false);
  printf("}\n");
}

std::vector<TaskSpec> on_leaves(const Model& M, const std::vector<int>& rows) {
  std::vector<TaskSpec> t;
  for (size_t i = 0; i < rows.size(); ++i) t.push_back({M.leaves[i % M.leaves.size()], -1, rows[i]});
  return t;
}

}  // namespace

// the models of a description file (see the head of this file), each planned once
int run_file(const char* path) {
  std::ifstream in(path);
  if (!in) { fprintf(stderr, "cannot read %s\n", path); return 1; }
  std::string line;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    std::istringstream ss(line);
    std::string name;
    int spheres = 0, n = 0, nt = 0, np = 0;
    ss >> name >> spheres >> n;
    std::vector<BodySpec> spec(n);
    for (BodySpec& b : spec) ss >> b.parent >> b.kind;
    Case c;
    c.name = "wide"; c.print_chain = true;
    ss >> nt;
    for (int t = 0; t < nt; ++t) { int body = 0; ss >> body; c.tasks.push_back({body, -1, 6}); }
    ss >> c.n_com >> np;
    c.pair_list.resize(2 * (size_t)np);
    for (int32_t& g : c.pair_list) ss >> g;
    if (!ss) { fprintf(stderr, "%s: malformed line for %s\n", path, name.c_str()); return 1; }
    for (int b = 0; b < n; ++b)
      if (spec[b].parent < 0 || spec[b].parent > b || spec[b].kind < FIXED || spec[b].kind > SLIDE) { fprintf(stderr, "%s: bad body %d\n", name.c_str(), b + 1); return 1; }
    for (const TaskSpec& t : c.tasks) if (t.body < 1 || t.body > n) { fprintf(stderr, "%s: bad task body\n", name.c_str()); return 1; }
    for (int32_t g : c.pair_list) if (g < 0 || g >= n) { fprintf(stderr, "%s: bad geom\n", name.c_str()); return 1; }
    Model M;
    make_model(M, name, spec, spheres != 0);
    HostModel hm;
    std::string err;
    if (plan_model(&M.flat, hm, err) != MKH_OK) { fprintf(stderr, "%s: %s\n", name.c_str(), err.c_str()); return 1; }
    run_case(M, hm, c);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1) return run_file(argv[1]);
  struct Entry { const char* name; std::vector<BodySpec> spec; };
  const std::vector<Entry> models = {
      {"chain6", chain(6)}, {"chain16", chain(16)}, {"chain17", chain(17)}, {"chain44", chain(44)}, {"chain63", chain(63)},
      {"chain64", chain(63, HINGE2)},                              // (64 dofs on 63 bodies: the wavefront kernels' last model)
      {"tree44", tree({9, 10, 9, 10})},                            // a humanoid's shape: free root, legs and arms
      {"tree62", tree({12, 13, 12, 13, 6})},                       // chains of 12 and 13 + 6 dofs: beyond the packed dof lists
      {"ball11", [] { auto s = chain(9); s[5].kind = BALL; return s; }()},
      {"chain68", chain(68)},                                      // beyond one wavefront
  };
  for (const Entry& e : models) {
    Model M;
    make_model(M, e.name, e.spec);
    HostModel hm;
    std::string err;
    if (plan_model(&M.flat, hm, err) != MKH_OK) { fprintf(stderr, "%s: %s\n", e.name, err.c_str()); return 1; }
    const int nv = hm.nv, leaf = M.leaves.back();
    std::vector<Case> cases;
    auto add = [&](const char* name, std::vector<TaskSpec> tasks) -> Case& {
      Case c; c.name = name; c.tasks = std::move(tasks); cases.push_back(c); return cases.back();
    };
    // 1, 3, 4 and 16 frame tasks with 6 / 5 / 3 active rows; n_jrows = 18, 19, 24, 25 (kMu, kMuBig and one past each)
    add("t1_r6", on_leaves(M, {6}));
    add("t1_r5", on_leaves(M, {5}));
    add("t1_r3", on_leaves(M, {3}));
    add("t3_rows18", on_leaves(M, {6, 6, 6}));
    add("t4_rows18", on_leaves(M, {6, 6, 3, 3}));                  // (tree44: feet 6 rows, palms 3 — the headline's shape)
    add("t4_rows19", on_leaves(M, {6, 5, 5, 3}));
    add("t4_rows24", on_leaves(M, {6, 6, 6, 6}));
    add("t5_rows25", on_leaves(M, {6, 6, 5, 5, 3}));
    add("t16_r3", on_leaves(M, std::vector<int>(16, 3)));
    add("t16_r6", on_leaves(M, std::vector<int>(16, 6)));
    add("t3_rows18_norefine", on_leaves(M, {6, 6, 6})).diag = MKH_DIAG_NO_COLD_REFINE;
    add("t1_r6_com", on_leaves(M, {6})).n_com = 1;
    add("t3_rows15_com", on_leaves(M, {6, 6, 3})).n_com = 1;
    // 8, 9 and 64 − nv + 1 capsule pairs; the cylinder against the box (general convex routine: the two-kernel split)
    for (int np : {8, 9, 64 - nv + 1})
      if (np > 0) add(("t1_r6_pairs" + std::to_string(np)).c_str(), on_leaves(M, {6})).n_pairs = np;
    add("t2_rows9_pairs8", on_leaves(M, {6, 3})).n_pairs = 8;
    add("t1_r6_cylbox", on_leaves(M, {6})).cylbox = true;
    // analytic pairs beyond planes / spheres / capsules: the low-rank start with half-space rows, alone and behind tight rows
    add("t2_rows9_boxpairs4", on_leaves(M, {6, 3})).n_boxpairs = 4;
    add("t2_rows9_boxpairs21", on_leaves(M, {6, 3})).n_boxpairs = 21;
    add("t1_r6_relative", {{leaf, 1, 6}});
    add("t1_r6_dense", on_leaves(M, {6})).dense = true;
    // (task, dof) pair lanes at their capacities: tasks on bodies whose chains add up to 64 / 65 and to 256 / 257 dofs
    if (std::string(e.name) == "chain16") add("dpairs64", {{16, -1, 3}, {16, -1, 3}, {16, -1, 3}, {16, -1, 3}});
    if (std::string(e.name) == "chain17") add("dpairs65", {{17, -1, 3}, {16, -1, 3}, {16, -1, 3}, {16, -1, 3}});
    if (std::string(e.name) == "chain44") {
      // (one row each: with more, the layout of 6 task blocks and their rows would cost the low-rank start its residency)
      add("jpairs256", {{43, -1, 1}, {43, -1, 1}, {43, -1, 1}, {43, -1, 1}, {42, -1, 1}, {42, -1, 1}});
      add("jpairs257", {{43, -1, 1}, {43, -1, 1}, {43, -1, 1}, {43, -1, 1}, {43, -1, 1}, {42, -1, 1}});
    }
    // lists of limits: 2 and 4 terms of each box kind (and one kind alone), two posture tasks; with capsule pairs (the wide
    // arrays of a model within one wavefront are only built behind half-space rows) split over two collision limits
    add("lim_c2_v2", on_leaves(M, {6})).lists(2, 2);
    add("lim_c4_v4", on_leaves(M, {6, 3})).lists(4, 4);
    add("lim_c3_v0", on_leaves(M, {6})).lists(3, 0);
    add("lim_c0_v3", on_leaves(M, {6})).lists(0, 3);
    add("lim_c2_v2_col2", on_leaves(M, {6})).lists(2, 2, 2).n_pairs = 5;
    add("lim_c4_v4_col2", on_leaves(M, {6})).lists(4, 4, 2).n_pairs = 4;
    // refused descriptors
    add("bad_cfg5", on_leaves(M, {6})).lists(5, 1);
    add("bad_vel5", on_leaves(M, {6})).lists(1, 5);
    add("bad_dof_range", on_leaves(M, {6})).bad = BAD_DOF_RANGE;
    add("bad_cost", on_leaves(M, {6})).bad = BAD_COST;
    add("bad_frame_id", on_leaves(M, {6})).bad = BAD_FRAME_ID;
    if (hm.jnt_type[hm.dof_jntid[0]] == JNT_FREE) add("bad_free_limit", on_leaves(M, {6})).bad = BAD_FREE_LIMIT;
    if (std::string(e.name) == "ball11") add("bad_ball_slots", on_leaves(M, {6})).bad = BAD_BALL_SLOTS;
    for (const Case& c : cases) run_case(M, hm, c);
  }
  return 0;
}
