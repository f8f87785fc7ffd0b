// The collision checker's host side (checker_host.hip), as the checked entry points of minkhip.hip see it: two refusals and the
// five stages that run a checker handle on a call's Stager.  Which buffer a stage goes through, in chunks of how many items and
// behind which pre-pass is its own business (checker_plan.h decides, checker_host.hip launches).
#pragma once
#include "checker_plan.h"
#include "host_internal.h"
#include "outer_launch.h"

namespace mkh {

// An attached checker in front of an entry point that would not run it.
int32_t refuse_checker(const MkhProblem* p, const char* who);
// Whether `ck` can serve the use `u` of a checked call on problem `p`: same device, same model, then the plan's refusal.
int32_t sweep_refuse_for(const MkhProblem* p, const MkhProblem* ck, const char* who, const CheckerUse& u);

// The clearance of N device rows on st's stream.  Every output is optional; status: MKH_ST_IN_COLLISION OR-ed in.
void clearance_rows(Stager& st, MkhProblem* ck, size_t N, const double* d_q, double* margin, int32_t* pair, int32_t* n_violated,
                    double* distance, int32_t* status);
// The sweep of a's edges (a.first, a.count, a.cv and a.n_cv are the stage's to fill).
void sweep_edges(Stager& st, const MkhProblem* ck, SweepArgs a);
// The certified sweep of a's edges in a's mode, one launch (a.reach is the stage's to fill: the checker's reach table, filled and
// uploaded at the handle's first use — a failure of that upload is latched like a failed launch).
void certify_edges(Stager& st, MkhProblem* ck, CertifiedArgs a);
// The check of candidate tracking over all T·B·S rows: node margins, the status bit, edge margins.
void tmf_check(Stager& st, const MkhProblem* ck, int B, int S, int T, int M, const double* q_all, const int32_t* cv_all, int32_t* st_all,
               double* nm_all, double* em_all);
// The check of one step of the refinement pass, between the loop launch of waypoint ct >= 0 and the step kernel that commits it.
void lr_check_step(Stager& st, const MkhProblem* ck, int B, int T, int M, int ct, int cdir, const LrWork& w, double* trip);

}  // namespace mkh
