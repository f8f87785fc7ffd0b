// The plain solve's host side (solve_host.hip), as the outer-loop calls of minkhip.hip see it: one record of a call and the one
// function that serves it.  Whether the call is refused, how its arrays travel and what is launched is its own business
// (solve_plan.h decides, solve_host.hip plans the launch and executes).
#pragma once
#include "host_internal.h"

namespace mkh {

// One plain solve.  The five entry points and the loop launches of the outer-loop calls fill what they need, by name; the rest
// keeps the value the entry points have always passed for it.
struct SolveCall {
  MkhProblem* p = nullptr;
  int32_t B = 0;
  const double* q = nullptr;                 // the handle's arguments: (B, nq), (B, n_frame, 7), posture and COM targets
  const double* frame_targets = nullptr;
  const double* posture_target = nullptr;
  const double* com_target = nullptr;
  double dt = 0.0, damping = 0.0;
  double* v_out = nullptr;                   // NULL: evaluation only (mkh_eval)
  int32_t* status_out = nullptr;
  const MkhTaps* taps = nullptr;
  int32_t flags = 0;
  void* hip_stream = nullptr;
  int32_t n_steps = 1;                       // fused loop: steps, or the most a threshold loop takes
  double* q_out = nullptr;                   // ... and where q ends
  const MkhDenseRows* dense = nullptr;
  double pos_threshold = -1.0, ori_threshold = -1.0;     // >= 0: the threshold-terminated loop
  int32_t* iters_out = nullptr;
  int32_t* converged_out = nullptr;
};

// Refusal, the warm-start state, then the call's arrays on their route and the launch.  A device-pointer call returns with its work
// enqueued on the call's stream; a host-pointer call returns with its outputs written.
int32_t solve(const SolveCall& c);

}  // namespace mkh
