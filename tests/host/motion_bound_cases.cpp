// Host-only driver of mink_amd/csrc/motion_bound.h for tests/test_certified_sweep_cpu.py: the reach table of hand-typed flat
// models — a planar chain of two hinges and a limited slide with a plane, a sphere, a capsule and a box; the same chain with the
// slide unlimited; the same chain with the plane on its last body; a ball with an anchor off the body origin above a body with a
// hinge and then a slide — one JSON object per line, infinities as the string "inf".  The
// arrays live in vectors of their exact size, so an index past an end is the address sanitizer's to report.  Built with the host
// sanitizers by the test and run as a child process.  Beside the tables: the two refusals of checker_plan.h for a certified sweep.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../../mink_amd/csrc/checker_plan.h"
#include "../../mink_amd/csrc/motion_bound.h"

namespace {

struct Flat {
  std::vector<int32_t> body_parentid{0, 0, 1, 2}, body_jntnum{0, 1, 1, 1}, body_jntadr{-1, 0, 1, 2};
  std::vector<double> body_pos{0, 0, 0, 0, 0, 0.5, 0.3, 0, 0, 0.4, 0, 0};
  std::vector<int32_t> jnt_type{3, 3, 2}, jnt_limited{0, 0, 1};
  std::vector<double> jnt_pos{0.1, 0, 0, 0, 0, 0.04, 0, 0, 0}, jnt_range{0, 0, 0, 0, -0.1, 0.2}, jnt_qpos0{0, 0, 0};
  std::vector<int32_t> geom_bodyid{0, 1, 2, 3}, geom_type{0, 2, 3, 6};       // floor (plane), sphere, capsule, box
  std::vector<double> geom_size{1, 1, 0.1, 0.05, 0, 0, 0.03, 0.1, 0, 0.03, 0.04, 0.12};
  std::vector<double> geom_pos{0, 0, 0, 0.2, 0, 0, 0.1, 0, 0, 0, 0, 0.05};
  mkh::MotionModel view() const {
    return mkh::MotionModel{(int)body_parentid.size(), (int)jnt_type.size(), body_parentid.data(), body_jntnum.data(),
                            body_jntadr.data(), body_pos.data(), jnt_type.data(), jnt_limited.data(), jnt_pos.data(), jnt_range.data(), jnt_qpos0.data(), geom_bodyid.data(), geom_type.data(),
                            geom_size.data(), geom_pos.data(), nullptr, nullptr, nullptr, nullptr};
  }
};

void print_table(const char* name, const Flat& f, const std::vector<int32_t>& pairs) {
  const int np = (int)pairs.size() / 2, njnt = (int)f.jnt_type.size();
  std::vector<double> out((size_t)np * njnt * 2, -1.0);
  mkh::motion_reach(f.view(), np, pairs.data(), out.data());
  printf("{\"case\": \"%s\", \"n_pairs\": %d, \"njnt\": %d, \"coef\": [", name, np, njnt);
  for (size_t i = 0; i < out.size(); ++i) {
    if (std::isinf(out[i])) printf("%s\"%sinf\"", i ? ", " : "", out[i] < 0 ? "-" : "");
    else printf("%s%.17g", i ? ", " : "", out[i]);
  }
  printf("]}\n");
}

void print_refusal(const char* name, const mkh::CheckerShape& s) {
  std::string err;
  const int32_t rc = mkh::checker_refuse(s, mkh::CheckerUse::certified(), "mkh_certified_sweep", err);
  printf("{\"case\": \"%s\", \"rc\": %d, \"err\": \"%s\", \"lds\": %zu}\n", name, rc, err.c_str(),
         mkh::certified_lds_bytes(s.nbody, s.nq, s.n_pairs));
}

}  // namespace

int main() {
  const std::vector<int32_t> pairs{0, 3, 1, 3, 2, 3, 0, 1};     // floor-box, sphere-box, capsule-box, floor-sphere
  Flat chain;
  print_table("chain", chain, pairs);
  Flat open = chain;
  open.jnt_limited[2] = 0;
  print_table("unlimited_slide", open, pairs);
  Flat carried = chain;
  carried.geom_bodyid[0] = 3;                                   // the plane rides on the last body
  print_table("plane_on_moving_body", carried, pairs);
  // STACK_MJCF of tests/test_tree_checker_cpu.py: a hinge, below it a ball whose anchor is off the body origin, below that a body
  // with a hinge and then a limited slide (four joints on three moving bodies); floor-box, sphere-box, capsule-box, floor-capsule
  Flat stack;
  stack.body_jntnum = {0, 1, 1, 2};
  stack.body_pos = {0, 0, 0, 0, 0, 0.5, 0.3, 0, 0, 0, 0.4, 0};
  stack.jnt_type = {3, 1, 3, 2};
  stack.jnt_limited = {0, 0, 0, 1};
  stack.jnt_pos = {0.1, 0, 0, 0, 0.03, 0.04, 0.06, 0, 0.08, 0.3, 0, 0};
  stack.jnt_range = {0, 0, 0, 0, 0, 0, -0.1, 0.2};
  stack.jnt_qpos0 = {0, 1, 0, 0};
  print_table("stack", stack, std::vector<int32_t>{0, 3, 1, 3, 2, 3, 0, 2});
  // {n_pairs, n_cv, convex_pairs, has_wide, nbody, nq, max_batch, sweep_rows, check_rows}
  print_refusal("served_quarter", mkh::CheckerShape{14, 0, false, true, 9, 6, 1, 0, 0});
  print_refusal("served_whole", mkh::CheckerShape{60, 0, false, true, 21, 20, 1, 0, 0});
  print_refusal("convex", mkh::CheckerShape{14, 1, true, true, 9, 6, 1, 0, 0});
  print_refusal("convex_with_sweep_rows", mkh::CheckerShape{14, 1, true, true, 9, 6, 1, 4096, 4096});
  print_refusal("lds_fits", mkh::CheckerShape{2708, 0, false, true, 7, 6, 1, 0, 0});      // 49 + 18 + 8124 = 8191 doubles
  print_refusal("lds_over", mkh::CheckerShape{2709, 0, false, true, 7, 6, 1, 0, 0});      // 49 + 18 + 8127 = 8194
  print_refusal("no_pairs", mkh::CheckerShape{0, 0, false, true, 9, 6, 1, 0, 0});
  return 0;
}
