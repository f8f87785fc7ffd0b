/*
 * minkhip.h — C ABI of libminkhip.so: batched differential IK on MI355X (gfx950).
 *
 * Drop-in boundary for the ONE hot path of kevinzakka/mink: `solve_ik` over a batch
 * of independent (q, target) instances.  The reference has no FFI of its own on
 * this path — it is a pure-Python plugin API that crosses into native code through
 * the third-party wheels `mujoco` (pybind11) and `quadprog` (Cython).  Every entry
 * point below therefore cites the reference *Python* interface it replaces
 * (file:line in /root/reference) and is what a ctypes binding of that interface
 * binds (see INTEGRATION.md for the binding a mink maintainer would add).
 *
 * Conventions
 *   - extern "C", plain pointers + sizes, no torch/numpy types.
 *   - every function returns MKH_OK (0) or a negative MKH_E_* code and never
 *     throws; mkh_last_error() gives a thread-local message.
 *   - arrays are float64 / int32, row-major, batch-major: q is (B, nq), v is (B, nv).
 *   - data pointers of the per-call functions are DEVICE pointers when
 *     MKH_FLAG_DEVICE_PTRS is set (e.g. torch.Tensor.data_ptr() on ROCm; the call
 *     is then asynchronous on `stream`), otherwise HOST pointers (the library
 *     stages through its own device buffers and returns after completion; from 32 MB
 *     of staged data on in up to four chunks whose copies run beside the kernels of their
 *     neighbours, on streams of the handle ordered by events against `stream`).
 *   - the library owns everything it allocates; the caller owns every buffer it
 *     passes.  One in-flight call per MkhProblem: asynchronous calls on one handle must be
 *     ordered (same stream, or events) — a handle carries the staging buffers and the ticket
 *     counter that hands the tail of a batch to idle wavefronts, so two of its launches running
 *     at the same time would corrupt each other.  Distinct problems are independent.  An MkhModel is shared by the
 *     problems created on it and by every caller of mkh_integrate: that entry point is re-entrant (its small host-pointer
 *     path stages through one buffer of the model under a mutex; every other path holds no state of the model).  A device-pointer
 *     call is one plain kernel launch with no host-side state: it can be captured into a hipGraph and
 *     replayed (tests/test_gpu_scale.py::test_launches_replay_inside_a_hip_graph).
 *   - per-instance `status` (int32): bit flags MKH_ST_*.
 */
#ifndef MINKHIP_H_
#define MINKHIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 106 (round 4): + mkh_geom_distance_eval; models beyond 64 bodies / dofs and instances with up to 448 active half-space rows
 * (the workgroup-per-problem kernel) where 105 returned MKH_E_LIMIT / MKH_ST_ROW_OVERFLOW.  No struct changed.
 * 107 (round 5): no signature or struct changed; calls that 106 refused now run — on models beyond 64 bodies / dofs the per-task
 * (e, J) and iteration taps (mkh_eval) and the fused loops mkh_solve_steps / mkh_solve_until; the fused loops and calls with taps
 * no longer report MKH_ST_ROW_OVERFLOW below 448 rows per instance (the flagged instances run again with every row).
 * 108 (round 6): + mkh_problem_create_diag and the MKH_DIAG_* bits (per-handle parity / measurement switches that used to be
 * MKH_DEBUG_* environment variables: the product library no longer reads its environment); MKH_ST_DEGENERATE documented.  No
 * struct and no existing signature changed.
 * Still 108: + mkh_solve_multistart and MkhMultistartIO (many starts per target, the best solution picked on the device).
 * Purely additive — no struct, signature, kernel or result of an existing entry point changed — so the number stays. */
#define MKH_VERSION 108

/* return codes */
#define MKH_OK 0
#define MKH_E_INVALID (-1)   /* bad argument / unsupported model feature   */
#define MKH_E_HIP (-2)       /* HIP runtime error (message has the detail)  */
#define MKH_E_NOGPU (-3)     /* no gfx950 device visible                    */
#define MKH_E_LIMIT (-4)     /* exceeds a size limit (16 frame tasks, ...).  Models beyond 64 bodies or 64 dofs run on the
                                workgroup-per-problem kernel, which keeps a problem's kinematic state in the 160 KB of LDS of one
                                CU: ≈ 8·(nq + 7·nbody + 6·njnt + 14·nv + 5.5·(nv + rows) + 64·frame tasks) bytes ≤ 158 KB — a
                                serial chain fits up to ≈ 550 dofs; mkh_problem_create reports the figure.  (mkh_model_create
                                itself refuses only beyond 4096 bodies / 1024 dofs.) */

/* per-instance status bits written to status_out */
#define MKH_ST_OK 0
#define MKH_ST_OUTSIDE_LIMITS 1  /* q violates a joint range by > 1e-6 (mink/configuration.py:77-110); still solved */
#define MKH_ST_INFEASIBLE 2      /* constraints inconsistent (quadprog "no solution" → mink/solve_ik.py:103 assert) */
#define MKH_ST_NOT_PD 4          /* H not positive definite (quadprog "matrix G is not positive definite") */
#define MKH_ST_ITER_LIMIT 8      /* active-set iteration cap hit */
#define MKH_ST_ROW_OVERFLOW 16   /* more half-space rows active at once than the solve could hold AND a row that found no place is
                                    violated at the solution.  No entry point returns it below 448 rows per instance: a wavefront
                                    kernel holds 64 - nv rows (the tightest contacts get them, the rest are checked at the
                                    solution), and the instances it flags are solved again with EVERY row by the
                                    workgroup-per-problem kernel — plain solves, calls with taps and (round 5) the fused loops
                                    mkh_solve_steps / mkh_solve_until, whose flagged instances run their whole loop again.  Beyond
                                    448 contacts in range the same rule applies one level up: the 448 tightest are rows, the bit
                                    is set only if a dropped one is violated at the solution; caller-defined limit rows that find
                                    no place set it unconditionally. */
#define MKH_ST_DEGENERATE 32     /* the active half-space rows of this instance were almost linearly dependent (many geom pairs of one
                                    body pair) and the answer comes from the tableau iteration, which loses digits there (errors up
                                    to ~1e-6 relative).  Transient: the workgroup-per-problem kernel behind every problem with rows
                                    re-solves such instances with orthogonal factors (quadprog's own algorithm) and clears the bit.
                                    A caller sees it only where that launch does not run: handles created with
                                    MKH_DIAG_NO_WIDE_REDO and calls that tap the cycle counters. */
#define MKH_ST_IN_COLLISION 64   /* set by the fan-out calls on a candidate whose final q is in collision, while a collision checker
                                    is attached (mkh_problem_set_collision_check, "THE RULE OF CLEARANCE" below).  No solve kernel
                                    sets it; like every bit but MKH_ST_OUTSIDE_LIMITS it makes a candidate ineligible. */

/* flags */
#define MKH_FLAG_DEVICE_PTRS 1   /* data pointers are device pointers; async on stream */
#define MKH_FLAG_POSTURE_BATCHED 2  /* posture_target is (B, nq) instead of (nq,)       */
#define MKH_FLAG_COM_BATCHED 4      /* com_target is (B, 3) instead of (3,)             */
#define MKH_FLAG_DIRECT_QP 8        /* never use the low-rank start of the QP (parity/diagnostic switch) */
#define MKH_FLAG_WAVE_KERNEL 16     /* never use the row- / lane-per-problem kernels of small robots (parity/diagnostic switch) */
#define MKH_FLAG_LANE_KERNEL 32     /* use the lane-per-problem kernel whenever the problem qualifies, whatever the batch
                                     * size (default: plain solves from 73728 instances, fused loops from 28672;
                                     * parity/diagnostic switch) */
#define MKH_FLAG_TWO_WAVES 64       /* never use the 3-waves-per-SIMD kernel variants (parity/diagnostic switch) */
#define MKH_FLAG_WARM_START 128     /* closed-loop callers: start the QP's active-set phase from where the previous solve of
                                     * THIS problem handle (same batch size, instance i = instance i) ended.  The state lives
                                     * in the handle; it is used from its third solve on and reset when the batch size
                                     * changes.  Same optimum as a cold solve (the QP is strictly convex), fewer pivots:
                                     * along an IK loop the active set changes by a few dofs per step.  Every kernel
                                     * family honours it: the wavefront kernels, the row kernel and (round 6) the lane kernel of
                                     * small robots; all keep their partition inside mkh_solve_steps / _until. */
#define MKH_FLAG_FULL_ROWS 512      /* collision problems: never launch the tight-rows variant first (fewer half-space rows than
                                     * geom pairs, the tightest contacts get them, flagged instances re-solved on the full-row
                                     * variant behind it) — parity/diagnostic switch */
#define MKH_FLAG_QUAD_KERNEL 256    /* use the row-per-problem kernel of small robots (16 lanes per problem, nv <= 16) whenever the problem
                                     * qualifies, whatever the batch size (default: plain solves below 73728 instances, fused
                                     * loops below 28672; the fused loops of a floating base under frame / posture tasks alone on
                                     * its two-row build, which the default leaves on the wavefront kernel; parity/diagnostic switch) */
#define MKH_FLAG_UNWIND_TURNS 1024  /* mkh_solve_multistart_set and mkh_solve_trajectory_ladder_nodes only: the loops' results are
                                     * moved to the full turn nearest the reference posture ("THE RULE OF THE UNWINDING") before
                                     * the distinct-set selection compares them.  Every other entry point refuses the bit with
                                     * MKH_E_INVALID. */

/* frame types (mink/constants.py:3 SUPPORTED_FRAMES) */
#define MKH_FRAME_BODY 0
#define MKH_FRAME_GEOM 1
#define MKH_FRAME_SITE 2

typedef struct MkhModel MkhModel;
typedef struct MkhProblem MkhProblem;
typedef struct MkhSeedTable MkhSeedTable;   /* "Seed tables" below */

/*
 * One-time flattened copy of the mjModel kinematic tree: the mjModel fields the
 * reference hot path reads (mink/configuration.py:53-155, limits/ constructors,
 * tasks/posture_task.py:44).  Field names/semantics are MuJoCo's.  Host pointers;
 * copied at mkh_model_create.
 */
typedef struct MkhFlatModel {
  int32_t nq, nv, nbody, njnt, ngeom, nsite;
  const int32_t *body_parentid, *body_rootid, *body_jntnum, *body_jntadr, *body_dofnum, *body_dofadr;
  const double *body_pos /*nbody*3*/, *body_quat /*nbody*4*/, *body_ipos /*nbody*3*/;
  const double *body_mass, *body_subtreemass;
  const int32_t *jnt_type, *jnt_qposadr, *jnt_dofadr, *jnt_bodyid, *jnt_limited;
  const double *jnt_pos /*njnt*3*/, *jnt_axis /*njnt*3*/, *jnt_range /*njnt*2*/, *qpos0 /*nq*/;
  const int32_t *dof_bodyid, *dof_jntid, *dof_parentid;
  const int32_t *site_bodyid;
  const double *site_pos /*nsite*3*/, *site_quat /*nsite*4*/;
  const int32_t *geom_bodyid, *geom_type;
  const double *geom_size /*ngeom*3*/, *geom_pos /*ngeom*3*/, *geom_quat /*ngeom*4*/;
  /* Mesh geoms (mjGEOM_MESH = 7) as mj_geomDistance sees them: their CONVEX HULL.  geom_dataid[g] = mesh of geom g (−1: not
   * a mesh geom); the hull vertices of mesh k, in the geom frame (the compiler re-expresses a mesh in its inertial frame and
   * folds that frame into geom_pos / geom_quat), are mesh_vert[3·mesh_vertadr[k] …), mesh_vertnum[k] of them — MuJoCo's
   * field names; from a real MjModel: the vertices mesh_graph lists (FlatModel.from_mjmodel).  nmesh = 0 / NULL pointers:
   * a model without mesh geoms.  A primitive FITTED to a mesh (<geom type="capsule" mesh=…>) is an ordinary primitive
   * here: its compiled geom_size / geom_pos / geom_quat say everything. */
  int32_t nmesh, nmeshvert;
  const int32_t *geom_dataid /*ngeom*/, *mesh_vertadr /*nmesh*/, *mesh_vertnum /*nmesh*/;
  const double *mesh_vert /*nmeshvert*3*/;
} MkhFlatModel;

/* mink.FrameTask(frame_name, frame_type, position_cost, orientation_cost, gain, lm_damping)
 * — mink/tasks/frame_task.py:29-46; cost = [position x3, orientation x3] (:60,:75). */
typedef struct MkhFrameTaskDesc {
  int32_t frame_type, frame_id;
  double cost[6];
  double gain, lm_damping;
  /* mink.RelativeFrameTask(frame, root, ...) — mink/tasks/relative_frame_task.py:28-48: pose of the
   * frame expressed in `root`; root_type < 0 selects the plain FrameTask (pose in the world).  The
   * task's target slot then holds transform_target_to_root. */
  int32_t root_type, root_id;
} MkhFrameTaskDesc;

/* mink.PostureTask(model, cost, gain, lm_damping) — mink/tasks/posture_task.py:29-52.
 * mink.DampingTask is the gain=0 special case (mink/tasks/damping_task.py:11-20). */
typedef struct MkhPostureTaskDesc {
  const double *cost /*nv*/;
  double gain, lm_damping;
} MkhPostureTaskDesc;

/* mink.ComTask(cost, gain, lm_damping) — mink/tasks/com_task.py:25-35 (subtree of body 1). */
typedef struct MkhComTaskDesc {
  double cost[3];
  double gain, lm_damping;
} MkhComTaskDesc;

/* mink.ConfigurationLimit(model, gain, min_distance_from_limits) —
 * mink/limits/configuration_limit.py:18-67.  lower/upper are the constructor's
 * per-qpos arrays (±mjMAXVAL where unlimited); indices are its dof `indices`.
 * A ball joint named by `indices` holds ONE value over its four qpos slots in lower and
 * in upper, as the constructor writes its range (the kernels rebuild the quaternion
 * (u, u, u, u) from it): slots that differ fail mkh_problem_create with MKH_E_INVALID.
 * Up to 4 configuration and 4 velocity limits per problem (MKH_E_LIMIT beyond). */
typedef struct MkhConfigurationLimitDesc {
  double gain;
  const double *lower /*nq*/, *upper /*nq*/;
  int32_t n_indices;
  const int32_t *indices;
} MkhConfigurationLimitDesc;

/* mink.VelocityLimit(model, velocities) — mink/limits/velocity_limit.py:33-69:
 * `indices` (dof ids) and `limit` (max |v|). */
typedef struct MkhVelocityLimitDesc {
  int32_t n_indices;
  const int32_t *indices;
  const double *limit;
} MkhVelocityLimitDesc;

/* mink.CollisionAvoidanceLimit(model, geom_pairs, gain, minimum_distance_from_collisions,
 * collision_detection_distance, bound_relaxation) — mink/limits/collision_avoidance_limit.py:145-185;
 * geom_id_pairs is the constructor's filtered (min,max) id list (:253-278).
 * Distance routines behind mj_geomDistance (:219): analytic for plane/sphere/capsule among themselves, box against
 * plane/sphere/capsule/box, cylinder against plane/sphere/capsule, plane–ellipsoid; every other pair of the convex
 * primitives sphere / capsule / ellipsoid / cylinder / box (cylinder–box, cylinder–cylinder, ellipsoid–*) through a
 * general convex distance routine (GJK on support mappings — MuJoCo uses libccd there).  A MESH geom takes part through its
 * convex hull (MkhFlatModel.mesh_vert): plane–mesh analytically (the hull's lowest vertex), mesh against any primitive or
 * mesh through the general convex routine with the hull's vertices as the support mapping.  Height fields — and mesh geoms
 * of a model that carries no hull for them — fail mkh_problem_create with MKH_E_INVALID.
 *
 * Two places where the contact differs from mujoco 3.1.6's by construction (no test against the wheel can exist here):
 *  (i) TIES.  Where the closest pair of points is not unique — a capsule parallel to a box face, face-to-face boxes —
 *      MuJoCo returns several contacts of equal distance and mj_geomDistance keeps the first of ITS enumeration.  The routines
 *      here: capsule ∥ box face — the midpoint of the stretch of the capsule's axis that lies over the face; parallel capsules —
 *      the two ends of the overlapping stretch as two contacts, the first kept (mjc_CapsuleCapsule's shape); boxes face to
 *      face — the first closest (vertex, face) pair in the routine's own vertex order.  The distance h is the same as MuJoCo's;
 *      the witness points feed mj_jac, so the row of G may differ by the lever arm between two equally close points.
 *      tests/test_gpu_collision_shapes.py::test_tie_rule_is_pinned holds these three rules in place.
 *  (ii) GENERAL CONVEX PAIRS.  The nine primitive pair types without an analytic routine, and every mesh pair, get the exact
 *      Euclidean distance of the two convex sets (GJK, ~1e-13) where MuJoCo answers with libccd's MPR on shapes inflated by
 *      half the margin each, to a tolerance of 1e-6: h agrees to that tolerance, not to 1e-9. */
typedef struct MkhCollisionLimitDesc {
  int32_t n_pairs;
  const int32_t *geom_id_pairs /*n_pairs*2*/;
  double gain, minimum_distance_from_collisions, collision_detection_distance, bound_relaxation;
} MkhCollisionLimitDesc;

/*
 * Plugin route: a caller-defined mink.Task subclass — anything that implements the reference's extension point
 * Task.compute_error / Task.compute_jacobian (mink/tasks/task.py:81-103) — reaches the device as DENSE ROWS: the
 * descriptor holds its constructor state (cost per row, gain, lm_damping: task.py:48-62), the per-call arrays hold
 * what its two methods return for every instance (MkhDenseRows).  The kernel folds them into the objective exactly
 * like Task.compute_qp_objective does (task.py:105-138): weighted rows W·J, weighted error W·(−gain·e),
 * H += (WJ)ᵀ(WJ) + lm_damping·‖W·(−gain·e)‖²·I, c −= (W·(−gain·e))ᵀ·WJ.
 */
typedef struct MkhDenseTaskDesc {
  int32_t k;            /* rows of compute_error / compute_jacobian */
  const double *cost;   /* (k,) */
  double gain, lm_damping;
} MkhDenseTaskDesc;

/* The task/limit lists solve_ik receives (mink/solve_ik.py:68-77).  The QP objective is a
 * sum, so list order only affects rounding; limits=[] disables limits, the Python layer
 * materialises mink's limits=None default (a fresh ConfigurationLimit, solve_ik.py:28-29). */
typedef struct MkhProblemDesc {
  int32_t n_frame_tasks;
  const MkhFrameTaskDesc *frame_tasks;
  int32_t n_posture_tasks;
  const MkhPostureTaskDesc *posture_tasks; /* each has its own target slot */
  int32_t n_com_tasks;
  const MkhComTaskDesc *com_tasks;
  int32_t n_configuration_limits;
  const MkhConfigurationLimitDesc *configuration_limits;
  int32_t n_velocity_limits;
  const MkhVelocityLimitDesc *velocity_limits;
  int32_t n_collision_limits;
  const MkhCollisionLimitDesc *collision_limits;
  /* plugin route (mkh_solve_dense): user Task subclasses, and the total number of rows G·Δq ≤ h that user Limit
   * subclasses return from Limit.compute_qp_inequalities (mink/limits/limit.py:34-57) */
  int32_t n_dense_tasks;
  const MkhDenseTaskDesc *dense_tasks;
  int32_t n_dense_limit_rows;
  /* 1: user Limit subclasses also contribute per-instance BOX rows (rows of G with a single nonzero entry — e.g. an
   * acceleration limit [I; −I] — folded by the caller into lo ≤ Δq ≤ hi): MkhDenseRows.limit_lo / limit_hi.  Box rows cost no
   * tableau row, so a limit with 2·nv of them fits any robot (general rows are capped at 64 − nv per instance). */
  int32_t dense_limit_box;
} MkhProblemDesc;

/* Per-call arrays of the plugin route (same host/device pointer convention as q).  K = Σ k over the dense tasks (in
 * descriptor order), M = n_dense_limit_rows.  A limit row with h = +inf is inactive (mink's Constraint.inactive,
 * limit.py:19-23, per row); at most 64 − nv rows (collision + dense) can be active in one instance.  A row of zeros with
 * h ≥ 0 is a row like any other: it holds a place and never binds.  limit_lo / limit_hi are intersected with the built-in box; single-entry rows that contradict each other (or the
 * box) arrive as limit_lo > limit_hi on that dof and give MKH_ST_INFEASIBLE with v = NaN, as the reference's QP would
 * (tests/test_gpu_qp_degenerate.py). */
typedef struct MkhDenseRows {
  const double *task_e; /* (B, K)      compute_error per instance                    */
  const double *task_J; /* (B, K, nv)  compute_jacobian per instance                 */
  const double *limit_G;/* (B, M, nv)  compute_qp_inequalities(...).G per instance   */
  const double *limit_h;/* (B, M)      compute_qp_inequalities(...).h per instance   */
  const double *limit_lo;/* (B, nv) or NULL: per-instance lower bounds on Δq from single-entry rows (−inf = none);   */
  const double *limit_hi;/* (B, nv) or NULL: upper bounds; both need MkhProblemDesc.dense_limit_box = 1             */
} MkhDenseRows;

/* Optional debug/parity taps: any non-NULL pointer receives that intermediate for the
 * whole batch (same host/device convention as the other data pointers). */
typedef struct MkhTaps {
  double *xpos;      /* (B, nbody, 3)  data.xpos          (mink/configuration.py:63)  */
  double *xquat;     /* (B, nbody, 4)  data.xquat                                     */
  double *frame_pose;/* (B, n_frame_tasks, 7) wxyz_xyz, get_transform_frame_to_world (:157-185) */
  double *subtree_com;/*(B, 3)        data.subtree_com[1] (mink/tasks/com_task.py:82) */
  double *task_e;    /* (B, n_rows)   compute_error of frame tasks (6 each), posture (nv each), com (3 each) */
  double *task_J;    /* (B, n_rows, nv) compute_jacobian, same row order             */
  double *H;         /* (B, nv, nv)   build_ik(...).P   (mink/solve_ik.py:63)         */
  double *c;         /* (B, nv)       build_ik(...).q                                 */
  double *box_lo;    /* (B, nv)  merged box  lo <= dq <= hi  from Configuration/VelocityLimit rows */
  double *box_hi;    /* (B, nv)                                                        */
  double *coll_G;    /* (B, n_pairs, nv) CollisionAvoidanceLimit G rows (0 when inactive) */
  double *coll_h;    /* (B, n_pairs)     and h (+inf when inactive)                   */
  int32_t *qp_iters; /* (B,)  packed counters of the active-set phase after the unconstrained solve:
                      * bits 0-9 pivots (Goldfarb-Idnani selections when rows exist), 10-19 outer loop
                      * iterations / block steps, 20-29 rank-1 pivots */
  int64_t *cycles;   /* (B, 16): [0,8) shader-clock stamps at the kernel's phase boundaries, [8,16) cycles summed
                      * over the QP iterations: phase-0 publish, phase-0 pivot, GI select, GI publish, GI ratio
                      * test, GI pivot; [14] stamp at the end of the Jacobian-column loop (profiling) */
} MkhTaps;

int32_t mkh_version(void);
const char *mkh_last_error(void);
int32_t mkh_device_count(void);

/* Upload the flattened kinematic tree once: the mujoco.MjModel fields mink reads per solve through
 * Configuration.update / get_frame_jacobian (mink/configuration.py:53-64,112-155), the limits' constructors
 * (limits/configuration_limit.py:41-67, limits/velocity_limit.py:45-69) and the collision pair filter
 * (limits/collision_avoidance_limit.py:75-115). */
int32_t mkh_model_create(const MkhFlatModel *host_model, int32_t device, MkhModel **out);
void mkh_model_destroy(MkhModel *model);

/* Snapshot the Task/Limit plugin objects of one solve_ik call site (the `tasks` and `limits` arguments of
 * mink/solve_ik.py:68-77; constructor state of tasks/frame_task.py:29-46, relative_frame_task.py:28-52,
 * posture_task.py:29-52, com_task.py:25-35 and of the three limits) into a device descriptor. */
/* max_batch: the largest B any later call on this handle may pass — with host OR device pointers: it sizes everything the
 * handle owns per instance (staging buffers, the active sets kept for MKH_FLAG_WARM_START).  A call with B > max_batch
 * returns MKH_E_INVALID before anything is launched.
 * A handle owns device state its launches share (ticket counters, the workspace slices and the redo queue of the
 * workgroup-per-problem kernel, warm-start sets): calls on ONE handle must not overlap in time — one stream at a time, or
 * streams ordered by events.  Handles of the same model are independent of each other. */
int32_t mkh_problem_create(MkhModel *model, const MkhProblemDesc *desc, int32_t max_batch, MkhProblem **out);
/* The same with per-handle diagnostic switches (MKH_DIAG_* bits, 0 = mkh_problem_create).  They select among paths that return
 * the same optimum and exist for parity tests ("what does the first launch alone leave flagged?") and measurements (bench.py's
 * redo_instances); no counterpart in the reference (mink/solve_ik.py:68-105 has one path).  Unknown bits: MKH_E_INVALID. */
#define MKH_DIAG_NO_WIDE_REDO 1    /* problems with half-space rows: do not build / launch the workgroup-per-problem kernel behind the
                                      wavefront kernel — instances it would re-solve keep MKH_ST_ROW_OVERFLOW / _DEGENERATE / failures */
#define MKH_DIAG_NO_TIGHT_REDO 2   /* collision problems on the tight-rows build: do not launch the full-row build behind it */
#define MKH_DIAG_NO_COLD_REFINE 4  /* low-rank QP start: no second elimination for the bounds the unconstrained minimiser violates */
#define MKH_DIAG_NO_PAIR_CULL 8    /* more than 64 collision pairs: no bounding-sphere cull in front of the distance routines */
int32_t mkh_problem_create_diag(MkhModel *model, const MkhProblemDesc *desc, int32_t max_batch, int32_t diag,
                                MkhProblem **out);
void mkh_problem_destroy(MkhProblem *problem);
int32_t mkh_problem_num_task_rows(const MkhProblem *problem);
int32_t mkh_problem_num_collision_pairs(const MkhProblem *problem);
/* Name of the kernel variant the last solve/eval on this handle launched ("" before the first call):
 * "ik_solve_kernel_<rows>_<features>[_r<dof rows>]".  Diagnostic (benchmarks, profiles). */
const char *mkh_problem_last_kernel(const MkhProblem *problem);

/*
 * Batched mink.solve_ik (mink/solve_ik.py:68-105):
 *   v[b] = solve_ik(Configuration(model, q[b]), tasks(targets[b]), dt, "quadprog", damping, limits=limits)
 *   q              (B, nq)
 *   frame_targets  (B, n_frame_tasks, 7)  transform_target_to_world as wxyz_xyz (frame_task.py:77-83)
 *   posture_target (n_posture_tasks, nq) or (B, n_posture_tasks, nq) with MKH_FLAG_POSTURE_BATCHED
 *   com_target     (n_com_tasks, 3) or (B, n_com_tasks, 3) with MKH_FLAG_COM_BATCHED
 *   v_out          (B, nv)   velocity dq/dt
 *   status_out     (B,)      MKH_ST_* bits (may be NULL)
 */
int32_t mkh_solve(MkhProblem *problem, int32_t B, const double *q, const double *frame_targets,
                  const double *posture_target, const double *com_target, double dt, double damping,
                  double *v_out, int32_t *status_out, int32_t flags, void *hip_stream);

/*
 * Fused outer IK loop on the device — what mink's callers write around solve_ik
 * (examples/arm_ur5e_actuators.py:88-97, examples/arm_aloha.py:146-169):
 *   for _ in range(n_steps): v = solve_ik(cfg, ...); cfg.integrate_inplace(v, dt)
 * q stays on chip between steps.  q_out (B, nq) receives the final configuration (may alias q),
 * v_out the last velocity, status_out the OR of the per-step status bits; an instance stops at the
 * first step whose QP fails.
 */
int32_t mkh_solve_steps(MkhProblem *problem, int32_t B, const double *q, const double *frame_targets,
                        const double *posture_target, const double *com_target, double dt, double damping,
                        int32_t n_steps, double *q_out, double *v_out, int32_t *status_out, int32_t flags,
                        void *hip_stream);

/*
 * mkh_solve / mkh_eval for a problem with dense (plugin) rows: same arguments plus the per-call dense arrays.
 * `taps` may be NULL (plain solve); task_e / task_J tap rows of the dense tasks follow the built-in ones.
 */
int32_t mkh_solve_dense(MkhProblem *problem, int32_t B, const double *q, const double *frame_targets,
                        const double *posture_target, const double *com_target, const MkhDenseRows *dense, double dt,
                        double damping, double *v_out, int32_t *status_out, const MkhTaps *taps, int32_t flags,
                        void *hip_stream);

/*
 * The same loop as the reference's callers REALLY write it (examples/arm_ur5e_actuators.py:88-97,
 * examples/arm_aloha.py:146-169):
 *   for i in range(max_iters):
 *       v = solve_ik(cfg, ...); cfg.integrate_inplace(v, dt)
 *       err = task.compute_error(cfg)
 *       if norm(err[:3]) <= pos_threshold and norm(err[3:]) <= ori_threshold: break      (for every frame task)
 * per instance, in one launch.  The position (orientation) test of a frame task only counts when it has a nonzero
 * position (orientation) cost.  iters_out (B,) = iterations performed (1..max_iters), converged_out (B,) = 1 when the
 * loop ended on the thresholds; q_out / v_out / status_out as in mkh_solve_steps.  iters_out / converged_out may be NULL.
 */
int32_t mkh_solve_until(MkhProblem *problem, int32_t B, const double *q, const double *frame_targets,
                        const double *posture_target, const double *com_target, double dt, double damping,
                        int32_t max_iters, double pos_threshold, double ori_threshold, double *q_out, double *v_out,
                        int32_t *status_out, int32_t *iters_out, int32_t *converged_out, int32_t flags,
                        void *hip_stream);

/*
 * Multi-start IK: the loop of mkh_solve_until from n_seeds = S starts per target, the best solution picked on the device —
 * one call, no B·S rows over the bus.  No counterpart in the reference: it is what a caller writes around a local method
 * with box limits (which stops at a joint limit or a singularity for a good share of far targets) — draw starts, repeat the
 * targets, run the loop, keep the converged result closest to a reference posture.
 *
 * Instance layout: instance i = b·S + s (the seeds of a target are contiguous).  SEED 0 OF EVERY TARGET IS THE CALLER'S OWN
 * q[b], bit for bit: the result is never worse than mkh_solve_until from q.  The problem needs max_batch >= B·S.
 *
 * Random numbers.  u(rng_seed, t, s, k) in [0, 1) is a pure function of the call's rng_seed, the GLOBAL target index
 * t = target_index0 + b, the seed index s and a draw index k — no state, no dependence on launch shape, chunking or sharding
 * (a caller that splits its targets passes the offset of row 0 as target_index0).  With 64-bit wrapping arithmetic and
 *   mix(z):  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31)
 *   G = 0x9E3779B97F4A7C15
 *   h = mix(rng_seed + G);  h = mix((h ^ t) + G);  h = mix((h ^ ((s << 32) | k)) + G);  u = (h >> 11) * 2^-53
 * (the splitmix64 finaliser, three times; the top 53 bits make the double).
 *
 * Seeding rule for s >= 1, per joint (qa = jnt_qposadr; every sum below is a rounded product followed by a rounded sum, never
 * a fused multiply-add, so a restatement in numpy reproduces hinge / slide entries bit for bit):
 *   limited hinge / slide   range_lo + (range_hi - range_lo) * u(.., k = qa)
 *   unlimited hinge         (q[b][qa] - pi) + (2 pi) * u(.., k = qa)
 *   unlimited slide, free   the caller's value (a loose object or a floating base is not thrown around)
 *   ball                    z = 2 u1 - 1, r = sqrt(1 - z z), phi = (2 pi) u2, half = 0.5 (theta_max u3) with u1, u2, u3 =
 *                           u(.., k = qa), u(.., qa + 1), u(.., qa + 2) and theta_max = range[1] when limited, else pi:
 *                           quaternion (cos half, (r cos phi) sin half, (r sin phi) sin half, z sin half)
 * With io->seeds the caller's (B, S, nq) starts are used instead (row 0 of every target is still replaced by q[b]).
 *
 * Selection, per target: among the seeds whose loop converged with no failure bit (status & ~MKH_ST_OUTSIDE_LIMITS == 0) the one
 * with the smallest d = sum_k w_k ((q_s (-) q_ref)_k)^2, (-) = mj_differentiatePos at dt = 1 (the tangent-space difference),
 * q_ref = io->q_ref[b] or the caller's q[b], w = io->weights or ones; ties go to the lowest seed index.  If no seed converged the
 * result is seed 0's — what mkh_solve_until returns from q — with converged = 0.  A QP failure of one seed discards that seed;
 * it is not an error of the call.
 *
 * Pointers in MkhMultistartIO follow the call's convention (device pointers with MKH_FLAG_DEVICE_PTRS, else host); outputs must
 * not alias inputs or each other.  The per-target outputs are required, everything else may be NULL.
 */
typedef struct MkhMultistartIO {
  const double *seeds;      /* (B, S, nq) caller-defined starts, or NULL: drawn by the rule above                     */
  const double *q_ref;      /* (B, nq) reference posture of the selection, or NULL: q                                 */
  const double *weights;    /* (nv,) weights of the selection, or NULL: ones                                          */
  double *q_best;           /* (B, nq)  final configuration of the chosen seed                                        */
  double *v_best;           /* (B, nv)  its last velocity                                                             */
  int32_t *iters;           /* (B,)     its iteration count                                                           */
  int32_t *status;          /* (B,)     its MKH_ST_* bits                                                             */
  int32_t *converged;       /* (B,)     1 when a seed converged without a failure bit                                 */
  int32_t *seed_index;      /* (B,)     the chosen s (0 when nothing converged)                                       */
  int32_t *n_converged;     /* (B,)     how many of the S seeds converged without a failure bit                       */
  double *q_all;            /* (B*S, nq) optional: every instance's final configuration                               */
  int32_t *converged_all;   /* (B*S,)    optional: the loop's converged flag per instance                             */
  int32_t *iters_all;       /* (B*S,)    optional                                                                     */
  int32_t *status_all;      /* (B*S,)    optional                                                                     */
  double *seeds_out;        /* (B*S, nq) optional: the starts the loop ran from                                       */
} MkhMultistartIO;
int32_t mkh_solve_multistart(MkhProblem *problem, int32_t B, const double *q, const double *frame_targets,
                             const double *posture_target, const double *com_target, double dt, double damping,
                             int32_t max_iters, double pos_threshold, double ori_threshold, int32_t n_seeds,
                             uint64_t rng_seed, int64_t target_index0, const MkhMultistartIO *io, int32_t flags,
                             void *hip_stream);

/*
 * Distinct solution sets: up to K = n_solutions DIFFERENT solutions per target out of the S that multi-start's loops found,
 * instead of the one closest to the reference posture — the IK branches of a target, for robots without a closed form, picked
 * and deduplicated on the device: no B·S rows over the bus.  No counterpart in the reference.
 *
 * THE RULE OF THE SET (mkh_select_distinct; mkh_solve_multistart_set runs it on the results of its loops).
 * One target, S candidates q_0 .. q_{S-1}, K = n_solutions, r = min_distance, a reference posture q_ref and weights w.
 *   Eligible   multi-start's: the loop converged (converged != 0) and status & ~MKH_ST_OUTSIDE_LIMITS == 0.  For
 *              mkh_select_distinct: valid[s] != 0, every candidate when valid is NULL.
 *   Distance   multi-start's, the same device function: d(a, b) = sum_k w_k ((a (-) b)_k)^2, (-) = mj_differentiatePos at
 *              dt = 1, w = weights (nv,) or ones when NULL.  d_ref(s) = d(q_s, q_ref), a NaN or infinite value replaced by
 *              DBL_MAX (last among the eligible), as in multi-start's selection.
 *   For slot j = 0 .. K-1, while an eligible candidate is left uncovered:
 *     the REPRESENTATIVE of slot j is the uncovered eligible candidate with the smallest d_ref, ties to the lowest index;
 *     slot j then COVERS every not-yet-covered eligible candidate s with d(q_s, q_rep) <= r·r; a comparison with NaN is false,
 *     so such a candidate stays uncovered.  The representative itself is always covered, and so is every candidate whose row
 *     is a bitwise copy of the representative's, whatever the arithmetic of d gives for them (the quaternion product
 *     conj(q) q of a ball or free joint need not round to the identity);
 *     multiplicity[j] = the number of candidates covered in that step.
 *   The walk stops when no uncovered eligible candidate is left, or after K slots.
 * This is the greedy walk through the eligible candidates in ascending (d_ref, index) that keeps a candidate iff it is farther
 * than r from every candidate kept before it; the cover formulation is the one that runs in parallel.
 * Two solutions that differ by a full turn of an unlimited (or multi-turn) hinge are 2 pi apart in (-) and therefore DIFFERENT
 * solutions: for a planner they are — reaching one from the other is a full turn of that joint.  r = 0 merges exact
 * duplicates only.
 *
 * Outputs.  Per target: n_distinct (B,) the slots filled, at most K; n_converged (B,) the eligible candidates, as in
 * multi-start; n_uncovered (B,) the eligible candidates no slot covers — 0: the set is complete for these candidates.  Per slot:
 * q_set (B, K, nq), v_set (B, K, nv), iters / status / seed_index / multiplicity (B, K), distance (B, K) = the
 * representative's d_ref.  AN EMPTY SLOT (j >= n_distinct) holds candidate 0's row in q_set / v_set / iters / status — every
 * row is a valid configuration — with seed_index = -1, multiplicity = 0, distance = +inf.
 * INVARIANT: where n_converged > 0, slot 0 is bitwise what mkh_solve_multistart returns for the same arguments (q_best, v_best,
 * iters, status, seed_index); where n_converged == 0 every slot is empty and repeats what that call returns: seed 0's result.
 *
 * 1 <= n_solutions <= 64; min_distance >= 0 and finite; else MKH_E_INVALID.  At most 4 096 candidates per target (n_seeds, S:
 * their state during the selection, 12 bytes each, lives in the LDS of the target's wavefront): beyond, MKH_E_LIMIT.
 *
 * mkh_solve_multistart_set: seeding, an attached seed table, target fan-out, the loops, the flags and the pointer conventions
 * are mkh_solve_multistart's — the optional q_all / converged_all / iters_all / status_all / seeds_out are that call's, bitwise
 * — and THE RULE OF THE SET replaces its selection.  Every output but those five is required.
 * mkh_select_distinct: the rule alone over a caller's own candidates q_candidates (B, S, nq) — closed-form branches, the q_all of
 * an earlier call filtered again with another r, the rungs of mkh_solve_trajectory_ladder.  Of MkhSolutionSetIO it reads the
 * outputs q_set, seed_index, multiplicity, distance, n_distinct, n_uncovered (required) and n_converged (optional: the number of
 * valid candidates); the other fields are ignored.  q_ref (B, nq) is required.
 */
typedef struct MkhSolutionSetIO {
  const double *seeds;      /* (B, S, nq) caller-defined starts, or NULL: drawn by multi-start's rule                 */
  const double *q_ref;      /* (B, nq) reference posture of d_ref, or NULL: q                                         */
  const double *weights;    /* (nv,) weights of the distance, or NULL: ones                                           */
  double *q_set;            /* (B, K, nq) final configuration of every slot's representative                          */
  double *v_set;            /* (B, K, nv) its last velocity                                                           */
  int32_t *iters;           /* (B, K)   its iteration count                                                           */
  int32_t *status;          /* (B, K)   its MKH_ST_* bits                                                             */
  int32_t *seed_index;      /* (B, K)   its s; -1 in an empty slot                                                    */
  int32_t *multiplicity;    /* (B, K)   candidates the slot covers; 0 in an empty slot                                */
  double *distance;         /* (B, K)   its d_ref; +inf in an empty slot                                              */
  int32_t *n_distinct;      /* (B,)     slots filled                                                                  */
  int32_t *n_converged;     /* (B,)     eligible candidates                                                           */
  int32_t *n_uncovered;     /* (B,)     eligible candidates left uncovered after the last slot                        */
  double *q_all;            /* (B*S, nq) optional, as in MkhMultistartIO                                              */
  int32_t *converged_all;   /* (B*S,)    optional                                                                     */
  int32_t *iters_all;       /* (B*S,)    optional                                                                     */
  int32_t *status_all;      /* (B*S,)    optional                                                                     */
  double *seeds_out;        /* (B*S, nq) optional: the starts the loop ran from                                       */
} MkhSolutionSetIO;
int32_t mkh_solve_multistart_set(MkhProblem *problem, int32_t B, const double *q, const double *frame_targets,
                                 const double *posture_target, const double *com_target, double dt, double damping,
                                 int32_t max_iters, double pos_threshold, double ori_threshold, int32_t n_seeds,
                                 int32_t n_solutions, double min_distance, uint64_t rng_seed, int64_t target_index0,
                                 const MkhSolutionSetIO *io, int32_t flags, void *hip_stream);
int32_t mkh_select_distinct(MkhProblem *problem, int32_t B, int32_t S, const double *q_candidates, const int32_t *valid,
                            const double *q_ref, const double *weights, int32_t n_solutions, double min_distance,
                            const MkhSolutionSetIO *io, int32_t flags, void *hip_stream);

/*
 * Turn unwinding: an opt-in step IN FRONT of the rule of the set.  THE RULE OF THE SET above stays as it is — two solutions a
 * full turn apart are different solutions — and nothing changes by default.  A caller for whom the turn does not matter (a
 * joint that may be commanded to any turn within its range) asks for every candidate to be moved to the turn nearest a
 * reference posture first; the set then spends its K slots on IK branches, not on turns of one branch.
 *
 * THE RULE OF THE UNWINDING (mkh_unwind_turns; MKH_FLAG_UNWIND_TURNS runs it on the results of the loops).
 * TWO_PI = 6.283185307179586 (the double nearest 2 pi).  Every product and every sum below is rounded on its own, never fused —
 * the convention of multi-start's seeding rule, so a restatement in numpy reproduces the device bit for bit.
 *   A joint is ELIGIBLE when it is a hinge and either unlimited or range_hi - range_lo >= TWO_PI (the rounded difference).
 *   For an eligible joint, x = the row's value and r = the reference's value at its qposadr:
 *     quotient = (r - x) / TWO_PI;  k = rint(quotient), rounding half to even;
 *     k = 0 when x, r or the quotient is not finite, or |quotient| > 1e6;
 *     when the joint is limited:  while k > 0 and x + k·TWO_PI > range_hi: k -= 1;
 *                                 while k < 0 and x + k·TWO_PI < range_lo: k += 1;
 *     the result is x itself, bit for bit, when k == 0, else x + k·TWO_PI.
 *   Every other entry of the row — slides, the quaternions and positions of ball and free joints, hinges that are not
 *   eligible — is a bit copy.
 * Consequences.  (1) The map is idempotent, bitwise: the quotient of a result is within 1/2 of 0 up to rounding, a second
 * pass finds k = 0 — or a k that the limits cut back to 0 — and returns the value itself; an exact half (r - x = ±pi) rounds
 * to the even k = 0 and stays (only a quotient within rounding of k + 1/2 for a k != 0 can land on either side of the half
 * after its shift).  (2) A value inside its range stays inside: k is cut back until the shifted value is, and k = 0
 * returns x.  A value outside its range is not pulled in.  (3) The pose of the robot moves only by the rounding of the
 * shift: a hinge at x + 2 pi k is the hinge at x, and |k·TWO_PI - 2 pi k| <= 2.5e-16 |k|.  (4) The loop's flags are CARRIED OVER,
 * not re-evaluated: a row that converged counts as converged after the unwinding, its status, iteration count and velocity
 * are the loop's.
 *
 * mkh_unwind_turns: the rule alone.  q_rows (n_rows, nq); row i is unwound toward q_ref[i / rows_per_ref], q_ref
 * (ceil(n_rows / rows_per_ref), nq); q_out (n_rows, nq) may be q_rows itself (in place).  n_rows >= 1, rows_per_ref >= 1.  Pointers
 * are host pointers (staged, synchronous) or device pointers with MKH_FLAG_DEVICE_PTRS (asynchronous on the stream); no other
 * flag bit is accepted.
 *
 * MKH_FLAG_UNWIND_TURNS on mkh_solve_multistart_set: the B·S loop results are unwound toward q_ref[b] (io->q_ref, or q when NULL)
 * in the workspace between the loops and the selection.  q_all then returns the UNWOUND rows; seeds_out, converged_all,
 * iters_all and status_all are unchanged.  The set's invariant "slot 0 is bitwise what mkh_solve_multistart returns" then holds
 * MODULO THE UNWINDING of that row: slot 0 is the closest unwound candidate, which need not be the closest raw one.
 */
int32_t mkh_unwind_turns(MkhProblem *problem, int32_t n_rows, int32_t rows_per_ref, const double *q_rows, const double *q_ref,
                         double *q_out, int32_t flags, void *hip_stream);

/*
 * Goal sets: multi-start IK to the BEST of G = n_goals candidate poses per target — the grasp poses of an object, the poses a
 * placement accepts, the yaws of a tool that is symmetric about its axis — instead of to one pose: which of the goals the robot
 * reaches, and the configuration of the one closest to the reference posture, picked on the device: no B·G·S rows over the bus.
 * No counterpart in the reference.
 *
 * THE RULE OF THE GOAL SET (mkh_select_goalset; mkh_solve_goalset runs it on the results of its loops), in multi-start's terms.
 * Shapes.  Target b has G goals and S = n_seeds starts per goal; instance i = (b·G + g)·S + s.  frame_targets (B, G, n_frame, 7);
 *   posture_target / com_target (n, w), or (B, G, n, w) with MKH_FLAG_POSTURE_BATCHED / MKH_FLAG_COM_BATCHED, as in the ladder.
 * Loops.  mkh_solve_multistart's on the B·G flattened (target, goal) pairs: q[b] is repeated G times, so seed 0 of EVERY goal
 *   is the caller's q[b], bit for bit; drawn seeds use the global target index (target_index0 + b)·G + g; a caller's seeds are
 *   (B, G, S, nq); an attached seed table is queried with every goal's own frame targets.  The loops run in chunks of whole
 *   goals, at most max_batch loops each, like the ladder's rungs: the call needs only max_batch >= S.
 * Level 1, per goal.  Multi-start's selection, unchanged: among the eligible seeds (converged != 0 and
 *   status & ~MKH_ST_OUTSIDE_LIMITS == 0; for mkh_select_goalset: valid[b, g, s] != 0, every candidate when valid is NULL) the one
 *   with the smallest d_ref(s) = d(q_s, q_ref[b]) wins — the same device function, d(a, b) = sum_k w_k ((a (-) b)_k)^2, a NaN or
 *   infinite value replaced by DBL_MAX — ties to the lowest s.  A goal is VALID when goal_valid[b, g] != 0, always when
 *   goal_valid is NULL; it is REACHED when it is valid and has an eligible seed; d_ref(g) is its winner's d_ref.
 * Level 2, per target.  Among the reached goals the one with the smallest score = goal_cost[b, g] + d_ref(g) wins — one rounded
 *   addition, never fused; goal_cost NULL: zeros — ties to the lowest g.  A given goal_cost must be finite and >= 0: host
 *   pointers are checked (MKH_E_INVALID); behind MKH_FLAG_DEVICE_PTRS a NaN cost makes the goal lose every comparison (it still
 *   counts in n_reached; a target whose reached goals all have NaN costs returns as if nothing were reached).
 * Nothing reached.  The target's row is seed 0 of the lowest valid goal, of goal 0 when none is valid: converged = 0,
 *   seed_index = 0, score = +inf, goal_index = that goal, or -1 when no goal is valid.
 * Invalid goals still run their loops — the launch shape does not depend on data — so their target rows must be valid poses:
 *   pad a ragged set by repeating one of its valid goals with goal_valid = 0.
 *
 * Outputs.  Per target: q_best (B, nq), v_best (B, nv), iters / status / converged / goal_index / seed_index / n_reached (B,),
 * score (B,).  Per goal: q_goal (B, G, nq), v_goal (B, G, nv), iters_goal / status_goal / seed_index_goal / reached /
 * n_converged_goal (B, G) (n_converged_goal: the eligible seeds, whatever goal_valid says), distance_goal (B, G) = d_ref(g),
 * +inf when the goal is not reached.  AN UNREACHED GOAL holds its seed 0's row, with seed_index_goal = 0 and reached = 0.  The
 * optional q_all / converged_all / iters_all / status_all / seeds_out are (B·G·S, .), as in MkhMultistartIO.
 * INVARIANTS.  (1) With G = 1 and goal_cost, goal_valid NULL the per-target outputs are bitwise mkh_solve_multistart's (its
 * n_converged is n_converged_goal).  (2) For any G, the per-goal outputs of valid goals are bitwise what mkh_solve_multistart
 * returns for the B·G flattened pairs — q repeated G times, q_ref likewise — at target_index0·G (reached is its converged).
 * (3) With goal_cost and goal_valid NULL, (goal_index, seed_index) is multi-start's selection over the G·S candidates of a
 * target taken as one flat list, index g·S + s.
 *
 * n_goals >= 1, n_seeds >= 1, every output above but the five optional ones: else MKH_E_INVALID, before a device is touched.  The
 * selection keeps no per-candidate state: the only cap is B·G·S <= 2^31 - 1 rows (MKH_E_LIMIT).
 *
 * mkh_solve_goalset: refusals, flags and pointer conventions are mkh_solve_multistart's.
 * mkh_select_goalset: the two levels alone over a caller's own candidates q_candidates (B, G, S, nq) — the closed-form branches
 * of every grasp — with valid (B, G, S) or NULL and q_ref (B, nq), required.  Of MkhGoalSetIO it reads goal_cost, goal_valid and
 * the outputs q_best, converged, goal_index, seed_index, n_reached, score, q_goal, seed_index_goal, reached, n_converged_goal,
 * distance_goal (required; n_converged_goal: the number of valid candidates); the velocity, iteration and status outputs and
 * every other field are ignored.
 */
typedef struct MkhGoalSetIO {
  const double *seeds;        /* (B, G, S, nq) caller-defined starts, or NULL: drawn by multi-start's rule              */
  const double *q_ref;        /* (B, nq) reference posture of d_ref, or NULL: q                                         */
  const double *weights;      /* (nv,) weights of the distance, or NULL: ones                                           */
  const double *goal_cost;    /* (B, G) finite, >= 0, or NULL: zeros                                                    */
  const int32_t *goal_valid;  /* (B, G) or NULL: every goal is valid                                                    */
  double *q_best;             /* (B, nq) final configuration of the chosen (goal, seed)                                 */
  double *v_best;             /* (B, nv) its last velocity                                                              */
  int32_t *iters;             /* (B,)    its iteration count                                                            */
  int32_t *status;            /* (B,)    its MKH_ST_* bits                                                              */
  int32_t *converged;         /* (B,)    1: a goal was reached and chosen                                               */
  int32_t *goal_index;        /* (B,)    the chosen g; nothing reached: the lowest valid goal, -1 when none is valid    */
  int32_t *seed_index;        /* (B,)    the chosen s; 0 when nothing is reached                                        */
  int32_t *n_reached;         /* (B,)    reached goals                                                                  */
  double *score;              /* (B,)    goal_cost + d_ref of the chosen goal; +inf when nothing is reached             */
  double *q_goal;             /* (B, G, nq) final configuration of every goal's winner (unreached: seed 0's)            */
  double *v_goal;             /* (B, G, nv) its last velocity                                                           */
  int32_t *iters_goal;        /* (B, G)  its iteration count                                                            */
  int32_t *status_goal;       /* (B, G)  its MKH_ST_* bits                                                              */
  int32_t *seed_index_goal;   /* (B, G)  its s; 0 when the goal is not reached                                          */
  int32_t *reached;           /* (B, G)  1: valid and an eligible seed                                                  */
  int32_t *n_converged_goal;  /* (B, G)  eligible seeds                                                                 */
  double *distance_goal;      /* (B, G)  d_ref of the winner; +inf when the goal is not reached                         */
  double *q_all;              /* (B*G*S, nq) optional, as in MkhMultistartIO                                            */
  int32_t *converged_all;     /* (B*G*S,)    optional                                                                   */
  int32_t *iters_all;         /* (B*G*S,)    optional                                                                   */
  int32_t *status_all;        /* (B*G*S,)    optional                                                                   */
  double *seeds_out;          /* (B*G*S, nq) optional: the starts the loops ran from                                    */
} MkhGoalSetIO;
int32_t mkh_solve_goalset(MkhProblem *problem, int32_t B, int32_t n_goals, const double *q, const double *frame_targets,
                          const double *posture_target, const double *com_target, double dt, double damping, int32_t max_iters,
                          double pos_threshold, double ori_threshold, int32_t n_seeds, uint64_t rng_seed, int64_t target_index0,
                          const MkhGoalSetIO *io, int32_t flags, void *hip_stream);
int32_t mkh_select_goalset(MkhProblem *problem, int32_t B, int32_t G, int32_t S, const double *q_candidates, const int32_t *valid,
                           const double *q_ref, const double *weights, const MkhGoalSetIO *io, int32_t flags, void *hip_stream);

/*
 * Trajectory IK: every instance follows its own time sequence of T waypoints, each solved from where the previous one ended —
 * what a caller writes as a loop of mkh_solve_until (motion retargeting, Cartesian path tracing, a horizon of goals), in one
 * call with nothing coming back to the host between waypoints.  No counterpart in the reference.
 *
 * For t = 0 .. T-1, every instance b runs the fused loop from q_{t-1}[b] (q_{-1} = q) against waypoint t's targets:
 *   pos_threshold >= 0 and ori_threshold >= 0   mkh_solve_until's loop with max_iters = n_steps
 *   pos_threshold <  0 and ori_threshold <  0   mkh_solve_steps' fixed count of n_steps; iters and converged must be NULL
 * (one threshold negative and the other not: MKH_E_INVALID).  q_traj[b, t], v_traj[b, t], status[b, t], iters[b, t] and
 * converged[b, t] are exactly what that loop returns: T launches of the same kernels, stream-ordered, bitwise the caller's loop.
 *
 * A FAILING WAYPOINT DOES NOT STOP THE TRAJECTORY.  A waypoint whose loop did not converge, or whose status carries a QP
 * failure bit, is reported in status[b, t] / converged[b, t] and nowhere else: waypoint t + 1 of that instance starts from
 * whatever q_out the loop left (an instance's loop stops at the first step whose QP fails), and the call returns MKH_OK.
 *
 * Layout.  Batch-major by default: frame_targets (B, T, n_frame, 7), outputs (B, T, .).  Posture targets are (n_posture, nq), or
 * (B, n_posture, nq) with MKH_FLAG_POSTURE_BATCHED; with posture_per_waypoint a T axis comes after B — (B, T, n_posture, nq) —
 * and leads when the target is not batched: (T, n_posture, nq).  The same rule holds for com_target with MKH_FLAG_COM_BATCHED and
 * com_per_waypoint.  With time_major = 1 the T axis moves to the front of every array of the call that has one: frame_targets
 * (T, B, n_frame, 7), posture (T, B, n_posture, nq), outputs (T, B, .); q stays (B, nq).  Time-major is the layout the loops run
 * on: with MKH_FLAG_DEVICE_PTRS they read the caller's target slabs and write the caller's output slabs directly — no extra
 * kernel, no copy, no workspace.  Batch-major arrays are transposed on the device before and after the loops.
 *
 * qvel (optional): qvel[b, t] = mj_differentiatePos(q_{t-1}[b], q_traj[b, t]) at waypoint_dt — per hinge / slide coordinate
 * (q_t - q_{t-1}) / waypoint_dt, a rounded difference followed by a rounded quotient, so that a numpy restatement reproduces it
 * bit for bit; free joint: the same for the three position coordinates, then, as for a ball joint, the rotation vector of
 * conj(q_{t-1}) q_t over waypoint_dt (mju_subQuat: body frame, angle in (-pi, pi]).
 *
 * MKH_FLAG_WARM_START is passed to every loop unchanged: the handle's warm state behaves as under T consecutive
 * mkh_solve_until calls with the flag.  Host pointers: inputs are staged once, the trajectory runs on the device, outputs come
 * back once at the end.  Outputs must not alias inputs or each other.  Every argument error is reported before any device work;
 * an error of a loop launch in mid-trajectory returns its code after the stream has drained.
 */
typedef struct MkhTrajectoryIO {
  double *q_traj;       /* (B, T, nq)  configuration at the end of every waypoint's loop                 required  */
  double *v_traj;       /* (B, T, nv)  last velocity of every waypoint's loop                            required  */
  int32_t *status;      /* (B, T)      MKH_ST_* bits of every waypoint's loop                            required  */
  int32_t *iters;       /* (B, T)      iterations performed; threshold mode only, may be NULL                     */
  int32_t *converged;   /* (B, T)      1 when the loop ended on the thresholds; threshold mode only, may be NULL  */
  double *qvel;         /* (B, T, nv)  optional: (q_t (-) q_{t-1}) / waypoint_dt, q_{-1} = q                      */
  double waypoint_dt;   /* > 0 when qvel is given                                                                 */
  int32_t posture_per_waypoint;   /* 0: the posture target is held over the trajectory; 1: it has a T axis        */
  int32_t com_per_waypoint;       /* the same for the CoM target                                                   */
  int32_t time_major;   /* 1: every (B, T, .) array of the call, inputs included, is (T, B, .) instead            */
} MkhTrajectoryIO;
int32_t mkh_solve_trajectory(MkhProblem *problem, int32_t B, int32_t T, const double *q, const double *frame_targets,
                             const double *posture_target, const double *com_target, double dt, double damping,
                             int32_t n_steps, double pos_threshold, double ori_threshold, const MkhTrajectoryIO *io,
                             int32_t flags, void *hip_stream);

/*
 * Keyframed trajectory IK: mkh_solve_trajectory whose T waypoint targets are interpolated on the device from K sparse
 * keyframes per instance — a motion clip recorded at 30-120 Hz and tracked at the solver's dt, a Cartesian move given as two
 * poses and a duration, a handful of via-points.  The keyframes cross the bus, not the waypoints, and the target workspace
 * of the handle does not grow with T.  No counterpart in the reference.
 *
 * THE RULE.  key_times (K) and waypoint_times (T) are HOST arrays shared by the batch, whatever `flags` says about the
 * other pointers.  key_times[0] < ... < key_times[K-1]; waypoint times are non-decreasing and every one lies inside
 * [key_times[0], key_times[K-1]].  A waypoint time outside that range, key times that do not increase, waypoint times that
 * decrease, or a NaN in either array: MKH_E_INVALID before any device work — no extrapolation, no silent clamping.
 *
 * For waypoint time tau the host picks the segment: k = the largest index with key_times[k] <= tau.
 *   k == K-1   the waypoint IS keyframe K-1, copied bit for bit
 *   otherwise  u = (tau - key_times[k]) / (key_times[k+1] - key_times[k]), in [0, 1): one rounded subtraction over one
 *              rounded subtraction, one rounded quotient
 *   u == 0     the waypoint IS keyframe k, copied bit for bit
 * For 0 < u < 1, between keyframes a = key[k] and b = key[k+1]:
 *   frame targets (wxyz_xyz)
 *     rotation     normalize(q_a * exp(u * log(q_a^-1 * q_b))) with the reference's SO3.log — sign-invariant, angle in
 *                  [0, pi]: the shortest arc whatever the sign of either quaternion — and SO3.exp, small-angle (Taylor)
 *                  branches included
 *     translation  p_a + u * (p_b - p_a): a rounded difference, a rounded product, a rounded sum, never an FMA
 *     Rotation and translation are blended apart (what a retargeting or Cartesian-move caller means), not along the SE3 screw.
 *   posture targets   q_a (+) u * (q_b (-) q_a), (-) = mj_differentiatePos at dt = 1, (+) = mj_integratePos:
 *     hinge / slide coordinates, free-joint positions   a + u * (b - a), rounded as above
 *     ball joints, free-joint rotations   mju_quatIntegrate(q_a, mju_quat2Vel(conj(q_a) * q_b, 1), u), then normalised
 *   CoM targets       a + u * (b - a), rounded as above
 * k and u are scalars of the kernel launches of waypoint t, which sit on the caller's stream directly in front of waypoint
 * t's loop launch and write ONE (B, .) slab per target group that every waypoint reuses.
 *
 * Layout.  frame_keys (B, K, n_frame, 7).  posture_keys / com_keys: with posture_keyframed = 0 the held target of
 * mkh_solve_trajectory — (n_posture, nq), or (B, n_posture, nq) with MKH_FLAG_POSTURE_BATCHED — and nothing is launched for
 * it; with posture_keyframed = 1 a K axis sits where posture_per_waypoint puts the T axis: (B, K, n_posture, nq) batched,
 * (K, n_posture, nq) otherwise.  The same for com_keys, com_keyframed and MKH_FLAG_COM_BATCHED.  With time_major = 1 the K
 * axis of every input and the T axis of every output lead: frame_keys (K, B, n_frame, 7), q_traj (T, B, nq).  Keyframes are
 * read in place through (instance, keyframe) strides: neither layout is transposed.
 *
 * frame_targets_out (B, T, n_frame, 7), posture_targets_out and com_targets_out (optional) receive the interpolated targets in
 * the layout mkh_solve_trajectory takes them in with the same flags, *_per_waypoint = *_keyframed and the same time_major:
 * the path the caller asked for.  posture_targets_out / com_targets_out must be NULL for a group that is held.  The call IS
 * mkh_solve_trajectory on those arrays: same launches of the same loops, bitwise the same outputs.
 *
 * Everything else — the waypoint loop, threshold / fixed-count modes, the failing-waypoint rule, MKH_FLAG_WARM_START, host /
 * device pointers, qvel over the uniform waypoint_dt, error ordering — is mkh_solve_trajectory's.
 */
typedef struct MkhKeyframeIO {
  double *q_traj;               /* (B, T, nq)  as MkhTrajectoryIO                                                 required  */
  double *v_traj;               /* (B, T, nv)                                                                     required  */
  int32_t *status;              /* (B, T)                                                                         required  */
  int32_t *iters;               /* (B, T)      threshold mode only, may be NULL                                             */
  int32_t *converged;           /* (B, T)      threshold mode only, may be NULL                                             */
  double *qvel;                 /* (B, T, nv)  optional: (q_t (-) q_{t-1}) / waypoint_dt, q_{-1} = q                        */
  double *frame_targets_out;    /* (B, T, n_frame, 7)  optional: the interpolated frame targets                             */
  double *posture_targets_out;  /* optional, posture_keyframed = 1 only: the interpolated posture targets                   */
  double *com_targets_out;      /* optional, com_keyframed = 1 only: the interpolated CoM targets                           */
  double waypoint_dt;           /* > 0 when qvel is given                                                                   */
  int32_t posture_keyframed;    /* 0: posture_keys is a held target; 1: it has a K axis                                     */
  int32_t com_keyframed;        /* the same for com_keys                                                                    */
  int32_t time_major;           /* 1: the K axis of every input and the T axis of every output lead                         */
} MkhKeyframeIO;
int32_t mkh_solve_keyframes(MkhProblem *problem, int32_t B, int32_t K, int32_t T, const double *q, const double *frame_keys,
                            const double *posture_keys, const double *com_keys, const double *key_times,
                            const double *waypoint_times, double dt, double damping, int32_t n_steps, double pos_threshold,
                            double ori_threshold, const MkhKeyframeIO *io, int32_t flags, void *hip_stream);

/*
 * Multi-start trajectory IK: mkh_solve_trajectory from n_seeds = S candidate starts per instance — S candidate trajectories,
 * each continuous by construction (waypoint t starts from the same candidate's waypoint t - 1) —, scored over the whole path,
 * one of them chosen and gathered on the device: one call, no B·S·T rows over the bus.  It is what a caller writes around
 * mkh_solve_trajectory when the path's first pose lies far from the current posture, or when the single start lands on an IK
 * branch that runs into a joint limit half-way along the path.  No counterpart in the reference.
 *
 * THE RULE.
 * Candidates.  Candidate i = b·S + s (the candidates of an instance are contiguous).  Their starts are mkh_solve_multistart's:
 * the same generator u(rng_seed, target_index0 + b, s, k), the same per-joint seeding rule, io->seeds (B, S, nq) as the
 * alternative.  CANDIDATE 0 OF EVERY INSTANCE STARTS AT THE CALLER'S OWN q[b], bit for bit: it is mkh_solve_trajectory's
 * trajectory.  The problem needs max_batch >= B·S.
 *
 * Tracking.  Every candidate follows the T waypoints of its instance exactly as mkh_solve_trajectory does on B·S instances
 * whose targets are those of instance b repeated S times: the same loops with the same flags (MKH_FLAG_WARM_START included),
 * the same target layouts, posture_per_waypoint, com_per_waypoint and time_major.  The repetition happens on the device:
 * waypoint t's (B, .) slab of a target group is fanned out into ONE (B·S, .) slab per group in front of waypoint t's loop,
 * reused by every waypoint (the target workspace does not grow with T).  A batched target that is held is fanned out once; a
 * target without a B axis is read where it is and launches nothing.  Threshold mode only: both thresholds >= 0, n_steps is
 * max_iters per waypoint (a fixed count leaves nothing to score: MKH_E_INVALID).  At least one frame task; no dense rows.
 *
 * Score, per candidate.  Waypoint t is TRACKED when converged[t] != 0 && (status[t] & ~MKH_ST_OUTSIDE_LIMITS) == 0.
 *   n_tracked = the number of tracked waypoints
 *   length    = sum over t = 0 .. T-1, in ascending t, of d(q_t, q_{t-1}), d(a, b) = sum_k w_k ((a (-) b)_k)^2 — multi-start's
 *               distance: (-) = mj_differentiatePos at dt = 1, w = io->weights or ones.  The weights
 *               must be >= 0 (a length is a sum of non-negative terms; one that comes out negative ranks last, like NaN).  Each d is computed as multi-start's
 *               selection computes it and added to the running sum, which starts at 0, by one rounded addition — never fused
 *               into the products inside d.  q_{-1} IS THE CALLER'S q[b] FOR EVERY CANDIDATE, not the seed: the jump from the
 *               current posture to the seed's first solution is part of what the robot pays.
 * Selection, per instance: (1) the largest n_tracked; (2) among those the smallest length, a length that is NaN or infinite
 * ranking behind every finite one; (3) among those the lowest s.  Nothing is discarded: a candidate that lost a waypoint can
 * win when none tracked more.  If no candidate tracked any waypoint, candidate 0 wins — mkh_solve_trajectory's result — and
 * n_tracked = 0.
 *
 * Outputs.  q_traj, v_traj, status, iters, converged: the chosen candidate's, in the call's layout ((B, T, .), or (T, B, .)
 * with time_major), bitwise rows of the loops.  seed_index (B,) the chosen s; n_tracked (B,) its count; n_complete (B,) how
 * many of the S candidates tracked all T waypoints; path_length (B,) its length.  qvel (optional, with waypoint_dt): the
 * chosen trajectory's, by mkh_solve_trajectory's rule with q_{-1} = q.  seeds_out (B·S, nq): the starts.  q_all (T, B·S, nq),
 * v_all (T, B·S, nv), status_all, iters_all, converged_all (T, B·S): every candidate's results, ALWAYS time-major whatever
 * time_major says — the layout the loops run on.
 *
 * Workspace.  The loops' results live in a workspace of the handle of T·B·S·((nq + nv)·8 + 12) bytes (q, v and three int32
 * per candidate and waypoint), grown on demand and kept; with MKH_FLAG_DEVICE_PTRS a given *_all array is written by the loops
 * directly and takes no workspace for that array.  Beside it: the starts (B·S·nq·8 bytes, or the caller's seeds_out) and one
 * (B·S, .) slab per fanned-out target group.  An allocation that fails: MKH_E_HIP, the message carries the size.
 *
 * n_seeds = 1 IS mkh_solve_trajectory: the same loop launches, bitwise the same outputs (seed_index = 0).  Pointers follow the
 * call's convention (device pointers with MKH_FLAG_DEVICE_PTRS, else host: inputs staged once, outputs back once at the end);
 * outputs must not alias inputs or each other.  Every argument error is reported before any device work; an error in
 * mid-trajectory returns its code after the stream has drained.
 */
typedef struct MkhTrajectoryMultistartIO {
  const double *seeds;      /* (B, S, nq) caller-defined starts, or NULL: drawn by multi-start's rule                        */
  const double *weights;    /* (nv,) weights of the path length, each >= 0, or NULL: ones                                    */
  double *q_traj;           /* (B, T, nq)  the chosen candidate's configurations                                   required  */
  double *v_traj;           /* (B, T, nv)  its last velocities                                                     required  */
  int32_t *status;          /* (B, T)      its MKH_ST_* bits                                                       required  */
  int32_t *iters;           /* (B, T)      its iteration counts                                                    required  */
  int32_t *converged;       /* (B, T)      its loops' converged flags                                              required  */
  int32_t *seed_index;      /* (B,)        the chosen s                                                            required  */
  int32_t *n_tracked;       /* (B,)        tracked waypoints of the chosen candidate                               required  */
  int32_t *n_complete;      /* (B,)        candidates that tracked all T waypoints                                 required  */
  double *path_length;      /* (B,)        length of the chosen candidate's path                                   required  */
  double *qvel;             /* (B, T, nv)  optional: (q_t (-) q_{t-1}) / waypoint_dt of the chosen path, q_{-1} = q          */
  double *seeds_out;        /* (B*S, nq)   optional: the starts the candidates ran from                                      */
  double *q_all;            /* (T, B*S, nq) optional: every candidate's configurations, time-major                           */
  double *v_all;            /* (T, B*S, nv) optional                                                                         */
  int32_t *status_all;      /* (T, B*S)    optional                                                                          */
  int32_t *iters_all;       /* (T, B*S)    optional                                                                          */
  int32_t *converged_all;   /* (T, B*S)    optional                                                                          */
  double waypoint_dt;       /* > 0 when qvel is given                                                                        */
  int32_t posture_per_waypoint;   /* as MkhTrajectoryIO                                                                      */
  int32_t com_per_waypoint;
  int32_t time_major;       /* 1: every (B, T, .) array of the call, inputs included, is (T, B, .) instead (not the *_all)   */
} MkhTrajectoryMultistartIO;
int32_t mkh_solve_trajectory_multistart(MkhProblem *problem, int32_t B, int32_t T, int32_t n_seeds, const double *q,
                                        const double *frame_targets, const double *posture_target, const double *com_target,
                                        double dt, double damping, int32_t n_steps, double pos_threshold, double ori_threshold,
                                        uint64_t rng_seed, int64_t target_index0, const MkhTrajectoryMultistartIO *io,
                                        int32_t flags, void *hip_stream);

/*
 * THE RULE, with a checker (mkh_select_trajectory_candidates; mkh_solve_trajectory_multistart_free runs it on the candidates it
 * tracks): the candidate whose waypoints AND motions are free of collision.  The terms are those of THE RULE above, of THE RULE OF
 * CLEARANCE and of THE RULE OF THE SWEEP (both further down), unchanged; the checker is an ARGUMENT of these calls, as for the
 * ladder.
 * Candidate i = b·S + s, waypoint t, rows q_all[t, i] (time-major, the layout the loops run on).
 *   Nodes.   node_margin(t, i) = the margin of q_all[t, i] by THE RULE OF CLEARANCE, for every row whatever its loop's flags.  A
 *            row in collision — !(margin >= 0), "a NaN decides" — gets MKH_ST_IN_COLLISION OR-ed into status_all[t, i], as the
 *            checked multi-start calls do.
 *            eligible(t, i) = converged_all[t, i] != 0 && (status_all[t, i] & ~MKH_ST_OUTSIDE_LIMITS) == 0, evaluated AFTER that OR.
 *   Edges.   For t >= 1 the edge into (t, i) runs from the same candidate's own row q_all[t - 1, i].  It is swept by THE RULE OF
 *            THE SWEEP with M = n_samples iff eligible(t, i); otherwise it is not swept and edge_margin(t, i) = NaN.  The start
 *            edge from q[b] is never swept, the ladder's convention: edge_margin(0, i) = +inf — IN THE _all ARRAY TOO, so that
 *            the chosen candidate's row is a plain gather.  This differs from the ladder's edge_margin_all, whose t = 0 entries
 *            are NaN.
 *   Score.   Waypoint t of a candidate counts as TRACKED iff eligible(t, i) && (t == 0 || edge_margin(t, i) >= 0).  Length,
 *            selection (count, then length, then lowest s), "nobody tracked anything: candidate 0" and n_complete are THE RULE
 *            above on these counts, unchanged.
 *   Loops.   Unchanged.  A candidate continues from its own waypoint t - 1 whatever the checker says; q_all, v_all, iters_all
 *            and converged_all are bitwise the unchecked call's, status_all differs by the one bit only.
 *   Outputs (MkhTrajectoryFreeIO), of the chosen candidate and in the call's layout ((B, T), or (T, B) with time_major):
 *            node_margin; edge_margin (entry 0 = +inf, NaN where the edge was not swept); edge_collision: 1 where t >= 1, the
 *            edge was swept and !(edge_margin >= 0); n_edge_collisions (B,).  Optional, ALWAYS time-major: node_margin_all and
 *            edge_margin_all (T, B·S).
 * Everything runs on the device: one launch over all T·B·S rows behind the last loop (a sweep has no per-row workspace), the
 * score, the gathers.  Both *_all margins live in a workspace of the PROBLEM handle of 2·T·B·S·8 bytes unless the caller's
 * device arrays take them.
 *
 * mkh_select_trajectory_candidates: the selection alone, over the caller's own candidates — q (B, nq) the current postures,
 * q_paths (T, B·S, nq) time-major, tracked (T, B·S) or NULL: every row.  checker NULL (free_io NULL iff checker NULL, else
 * MKH_E_INVALID): THE RULE above with "tracked != 0" as a waypoint's flag.  With a checker: tracked plays converged_all,
 * status_all is taken as 0, and the rule "with a checker" applies.  Outputs (B,): seed_index, n_tracked, n_complete,
 * path_length; optional q_path (B, T, nq), the chosen candidate's rows; with a checker the MkhTrajectoryFreeIO, (B, T).  Host
 * pointers (staged, synchronous) or device pointers with MKH_FLAG_DEVICE_PTRS (asynchronous on the stream); no other flag.  It
 * runs no loops: an attached checker is neither read nor refused, and B·S is not bound by max_batch; B·S·T < 2^31.
 *
 * mkh_solve_trajectory_multistart_free: mkh_solve_trajectory_multistart's arguments, refusals and pointer conventions, with the
 * checker, n_samples and the MkhTrajectoryFreeIO; it runs that call with the rule "with a checker" in place of the plain score.
 * A checker attached with mkh_problem_set_collision_check is still refused.  The checker must pass mkh_swept_clearance's
 * refusals (general convex pairs, the LDS slice), live on the problem's device and belong to its MkhModel (MKH_E_INVALID /
 * MKH_E_LIMIT); n_samples >= 1.  Every argument error is reported before any device work.  n_seeds = 1 is mkh_solve_trajectory's
 * rows, bitwise, plus the verdict.  "One call in flight per checker handle" holds.
 */
typedef struct MkhTrajectoryFreeIO {
  double *node_margin;         /* (B, T)    the clearance margin of the chosen candidate's rows                    required  */
  double *edge_margin;         /* (B, T)    the swept margin of the motion into each of them                       required  */
  int32_t *edge_collision;     /* (B, T)    1 where the motion into waypoint t was swept and collides              required  */
  int32_t *n_edge_collisions;  /* (B,)      colliding motions of the chosen candidate                              required  */
  double *node_margin_all;     /* (T, B*S)  optional: every row's clearance margin, time-major                               */
  double *edge_margin_all;     /* (T, B*S)  optional: every row's swept margin, time-major                                   */
} MkhTrajectoryFreeIO;
typedef struct MkhTrajectoryCandidatesIO {
  int32_t *seed_index;      /* (B,)        the chosen s                                                            required  */
  int32_t *n_tracked;       /* (B,)        tracked waypoints of the chosen candidate                               required  */
  int32_t *n_complete;      /* (B,)        candidates that tracked all T waypoints                                 required  */
  double *path_length;      /* (B,)        length of the chosen candidate's path                                   required  */
  double *q_path;           /* (B, T, nq)  optional: the chosen candidate's rows                                             */
} MkhTrajectoryCandidatesIO;
int32_t mkh_select_trajectory_candidates(MkhProblem *problem, MkhProblem *checker /* or NULL */, int32_t B, int32_t T, int32_t S,
                                         const double *q, const double *q_paths /* (T, B*S, nq) */,
                                         const int32_t *tracked /* (T, B*S) or NULL: all */, const double *weights,
                                         int32_t n_samples, const MkhTrajectoryCandidatesIO *io,
                                         const MkhTrajectoryFreeIO *free_io /* NULL iff checker NULL */, int32_t flags,
                                         void *hip_stream);
int32_t mkh_solve_trajectory_multistart_free(MkhProblem *problem, MkhProblem *checker, int32_t B, int32_t T, int32_t n_seeds,
                                             const double *q, const double *frame_targets, const double *posture_target,
                                             const double *com_target, double dt, double damping, int32_t n_steps,
                                             double pos_threshold, double ori_threshold, uint64_t rng_seed, int64_t target_index0,
                                             int32_t n_samples, const MkhTrajectoryMultistartIO *io,
                                             const MkhTrajectoryFreeIO *free_io, int32_t flags, void *hip_stream);

/*
 * Seed tables: multi-start seeded from the nearest stored postures.  The drawn starts of mkh_solve_multistart and
 * mkh_solve_trajectory_multistart are blind to the target; a seed table holds N postures keyed on the world poses their
 * frame-task frames reach, and a query returns, per target, the K stored postures whose poses are nearest — the way planners
 * start IK from a database.  A table is device memory of its own: it outlives the problem that made it and may be attached to
 * any problem of the same model, device and number of frame tasks, by several handles and threads at once (it is read-only
 * after mkh_seed_table_create).  No counterpart in the reference.
 *
 * Entries.  q_tab (N, nq).  Drawn (entries == NULL): entry j is row s = 1 of multi-start's seeding rule above at
 * (rng_seed, t = j, s = 1) around the one configuration q0 (nq,) — the same kernel, the same generator.  Free joints and
 * unlimited slides keep q0's value: the table of a floating-base robot belongs to q0's base pose.  Caller's entries: the
 * (N, nq) array as given (solutions of earlier calls, a teach-in set); q0 may then be NULL.
 *
 * Keys.  The world poses (wxyz, xyz) of the problem's n_frame frame-task frames at every entry: the frame_pose tap of mkh_eval
 * on the entries, evaluated in chunks of the problem's max_batch — a key is bitwise what mkh_eval says about that entry.
 * mkh_seed_table_read returns them as (N, n_frame, 7).
 *
 * Metric between a target T (n_frame, 7) and entry e, every product and sum rounded on its own (no fused multiply-add), in
 * this order:
 *   d = sum over f ascending, from 0, of ( wp_f * ((dx*dx + dy*dy) + dz*dz)  +  wo_f * max(0, 4 * (1 - c*c)) )
 *   (dx, dy, dz) = position of e's frame f - position of T's,  c = (((w w' + x x') + y y') + z z') / sqrt(n_T * n_e),
 *   n = ((w w + x x) + y y) + z z of either quaternion.
 * The orientation term is 4 sin^2(theta / 2) of the angle between the two rotations — theta^2 for small angles — and does not
 * change with the sign or the scale of either quaternion.  A d that is not finite (a NaN in the target: the max() keeps it)
 * counts as DBL_MAX, as in multi-start's selection.  Default weights (position in m^2, orientation in rad^2): wp_f = 1 when
 * any position cost of frame task f is > 0, else 0; wo_f likewise from its orientation costs; a RelativeFrameTask gets 0 / 0
 * (its target is no world pose).  pos_weight / ori_weight (n_frame,) replace them; each must be finite and >= 0, and all of
 * them 0 is refused, as is a problem whose default weights are all 0 (no plain FrameTask with a non-zero cost).
 *
 * Query.  Per target the K entries with the smallest (d, j) in lexicographic order — ties go to the lower entry index —
 * in ascending order: index_out (B, K), dist_out (B, K), and the entries' q as rows 1 .. K of seeds_out (B, K + 1, nq), whose
 * row 0 is left alone (it is the slab mkh_solve_multistart's io->seeds takes, where row 0 is replaced by q anyway).  The scan
 * is exact.  1 <= K <= 255 (else MKH_E_LIMIT above, MKH_E_INVALID below) and K <= N (MKH_E_INVALID); every output is optional
 * but one must be given.  Pointers are host pointers (synchronous), or device pointers with MKH_FLAG_DEVICE_PTRS
 * (asynchronous on the stream).  mkh_seed_table_create and mkh_seed_table_read take host pointers and are synchronous.
 *
 * Attached (mkh_problem_set_seed_table; NULL detaches): every mkh_solve_multistart and mkh_solve_trajectory_multistart call
 * on that handle WHOSE io->seeds IS NULL takes rows s >= 1 of every instance from the table — the n_seeds - 1 entries nearest
 * to the instance's frame targets (the trajectory call: waypoint 0's) — instead of drawing them: the query runs on the call's
 * stream directly in front of the seed kernel and writes the slab that kernel reads a caller's seeds from.  Seed 0 stays the
 * caller's q; io->seeds given: the caller's seeds win; rng_seed and target_index0 then do not enter the starts, so the result
 * depends on the targets alone.  n_seeds = 1 and no table attached: the call as it is without this section, bit for bit.
 * Refused with MKH_E_INVALID (MKH_E_LIMIT beyond 255 rows), the figure in the message: a table of another device, of another
 * model (nq, njnt) or of another n_frame; a problem without a plain FrameTask of non-zero cost; n_seeds - 1 > N.  The table
 * must stay alive while it is attached.
 */
int32_t mkh_seed_table_create(MkhProblem *problem, int32_t n_entries, const double *q0, const double *entries,
                              uint64_t rng_seed, const double *pos_weight, const double *ori_weight, MkhSeedTable **out);
void mkh_seed_table_destroy(MkhSeedTable *table);
int32_t mkh_seed_table_read(const MkhSeedTable *table, double *q_out /* (N, nq) or NULL */,
                            double *keys_out /* (N, n_frame, 7) or NULL */);
int32_t mkh_seed_table_query(const MkhSeedTable *table, int32_t B, const double *frame_targets, int32_t K,
                             int32_t *index_out, double *dist_out, double *seeds_out, int32_t flags, void *hip_stream);
int32_t mkh_problem_set_seed_table(MkhProblem *problem, const MkhSeedTable *table);

/*
 * Clearance: how far a batch of configurations is from collision, on the device — and, attached to a problem, the stage behind
 * the loops of the fan-out calls that takes colliding candidates out of their selections.  No counterpart in the reference: it is
 * the check a caller runs on the results of a global IK before using one (mj_geomDistance over a pair list at every candidate).
 *
 * A CHECKER is an ordinary MkhProblem whose descriptor has collision limits; its tasks and its other limits do not enter (a
 * descriptor with no tasks at all is accepted).
 *
 * THE RULE OF CLEARANCE (mkh_clearance; the fan-out calls run it on the final q of every candidate).
 *   Pair list  the checker's collision limits in descriptor order, each limit's geom_id_pairs in its own order: pair k carries
 *              dmin_k = minimum_distance_from_collisions and ddetect_k = collision_detection_distance of its limit; gain and
 *              bound_relaxation do not enter.
 *   For one row q (nq,):
 *   d_k        mj_geomDistance(geom1_k, geom2_k, distmax = ddetect_k) at the forward kinematics of q (quaternions normalised as
 *              mj_kinematics does), by the device routines of the collision phase: d_k <= ddetect_k, and a pair the
 *              bounding-sphere cull skips has d_k = ddetect_k — what mj_geomDistance says about it.
 *   margin     min_k (d_k - dmin_k)
 *   pair       the lowest k that attains the minimum
 *   n_violated #{k : !(d_k >= dmin_k)}
 *   The row is IN COLLISION iff !(margin >= 0).  A NaN decides: a row with a NaN term has margin = NaN and pair = the lowest k
 *   with a NaN term (numpy's min / argmin), and is in collision, never free.  A row of q with a NaN or an infinite entry has
 *   EVERY d_k = NaN, stated outright and not left to what the distance routines make of such poses (their clamps and range
 *   tests swallow a NaN): margin = NaN, pair = 0, n_violated = the number of pairs.
 *
 * mkh_clearance evaluates N rows in chunks of the checker's max_batch.  Pointers are host pointers (synchronous) or device
 * pointers with MKH_FLAG_DEVICE_PTRS (asynchronous on the stream); no other flag is accepted.  Refused with MKH_E_INVALID: a
 * checker without collision pairs; a checker created with MKH_DIAG_NO_WIDE_REDO (it has no per-body arrays to compute poses
 * from); general convex pairs (cylinder-box, ellipsoid-*, mesh hulls) on a checker whose model has more than 64 bodies or dofs
 * (they are not pre-evaluated there).  MKH_E_LIMIT beyond 1170 bodies (the poses of a row live in 64 KB of LDS).
 *
 * Attached (mkh_problem_set_collision_check; NULL detaches; the checker may be the problem itself: "the limit I solved with"):
 * mkh_solve_multistart, mkh_solve_multistart_set and mkh_solve_goalset run the clearance of every candidate's final q directly
 * behind their loops, on the call's stream, and OR MKH_ST_IN_COLLISION into the status row of every candidate that is in
 * collision.  Their selections then run on those rows unchanged — any status bit but MKH_ST_OUTSIDE_LIMITS makes a candidate
 * ineligible — so n_converged / n_reached count the candidates that converged AND are free.  q_all, iters_all and
 * converged_all are the loops' own; status_all carries the bit.  If nothing is eligible the result is seed 0's with
 * converged = 0, as without a checker; its status says so when seed 0 itself collides.  With a checker attached the call is
 * therefore NOT "never worse than mkh_solve_until from q": a converged seed 0 that collides is not returned as converged.
 * Every other entry point that runs loops over candidates or waypoints — mkh_solve_trajectory, mkh_solve_keyframes,
 * mkh_solve_trajectory_multistart, the three ladder calls and mkh_ladder_refine — returns MKH_E_INVALID while a checker is
 * attached (it would not be honoured).  The checker must live on the problem's device and belong to the same MkhModel
 * (MKH_E_INVALID otherwise), and must stay alive while it is attached.  The stage runs on the CHECKER handle's buffers (its
 * pre-evaluated convex pairs): "one call in flight per handle" holds for the checker too — two problems that share a checker,
 * or a problem and mkh_clearance on it, must not run at the same time on different streams.
 */
typedef struct MkhClearanceIO {
  double  *margin;      /* (N,)  required */
  int32_t *pair;        /* (N,)  required */
  int32_t *n_violated;  /* (N,)  required */
  double  *distance;    /* (N, n_pairs) optional: every d_k */
} MkhClearanceIO;
int32_t mkh_clearance(MkhProblem *checker, int32_t N, const double *q_rows /* (N, nq) */, const MkhClearanceIO *io,
                      int32_t flags, void *hip_stream);
int32_t mkh_problem_set_collision_check(MkhProblem *problem, MkhProblem *checker /* or NULL */);

/*
 * Swept clearance: whether the MOTION between two configurations is free of collision, not only its two ends — the check a
 * planner runs on every edge of a joint-space path.  The straight joint-space move is sampled at M interior points and every
 * sample is judged by THE RULE OF CLEARANCE; the samples are built and evaluated on the device and never written to memory.
 *
 * THE RULE OF THE SWEEP (mkh_swept_clearance; the checked ladder calls run it on the edges of their graph).
 * For an edge from row a to row b (nq each) and M = n_samples >= 1:
 *   Samples        u_i = i / (M + 1) for i = 1 .. M (one division of doubles): interior points — the ends are nodes and are
 *                  judged as nodes.  q(u) = a (+) u (b (-) a) per joint type, exactly the posture rule of mkh_solve_keyframes:
 *                  scalars a + u (b - a) — a difference, a product, a sum, contraction off —, quaternions by
 *                  mju_quatIntegrate(a, mju_subQuat(b, a), u): the shortest arc whatever the sign of either quaternion.
 *   Sample margin  m_i = margin(q(u_i)) by THE RULE OF CLEARANCE, unchanged: the pair list, the ddetect cap, the cull, "a NaN
 *                  decides".
 *   Edge outputs   margin = min_i m_i; sample = the lowest i - 1 that attains it; pair = the pair of that sample's clearance —
 *                  numpy's min / argmin, a NaN sample deciding as a NaN term does (the first one).
 *   The edge COLLIDES iff !(margin >= 0).
 *   A NaN or an infinity in a or b makes EVERY sample NaN: margin = NaN, sample = 0, pair = 0, the edge collides.
 *
 * mkh_swept_clearance evaluates N edges, q_from and q_to (N, nq); every output is (N,) and required.  Host pointers
 * (synchronous; staged whole) or device pointers with MKH_FLAG_DEVICE_PTRS (asynchronous on the stream); one launch either way —
 * a sweep has no per-row workspace, so N is not bound by the checker's max_batch; no other flag is accepted.  The checker is refused as mkh_clearance refuses it, and in addition:
 * General convex pairs.  A checker WITH general convex pairs (cylinder-box, ellipsoid-*, mesh hulls) is refused with
 * MKH_E_INVALID by every sweep entry point by default: those pairs are pre-evaluated on rows in memory, and a sweep has none.
 * mkh_problem_set_sweep_rows(checker, rows) reserves what lifts the refusal for mkh_swept_clearance, mkh_ladder_select_free and
 * mkh_solve_trajectory_ladder_free (with and without n_nodes): a device buffer of `rows` sample rows, one distance (8 bytes)
 * per general convex pair and row.  Such a call then walks its edges in chunks of floor(rows / n_samples) edges; per chunk the
 * general convex routine runs on every interior sample of the swept edges with finite ends — the sample's q(u) formed joint by
 * joint with the arithmetic above, the same doubles the analytic pairs see — and the sweep reads the distances; the stream
 * orders the reuse of the buffer.  THE RULE does not change: a sample is judged as mkh_clearance judges a row, and the outputs do
 * not depend on `rows`.  rows < n_samples (less than one edge) on a checker with general convex pairs: MKH_E_LIMIT.  On a
 * checker without such pairs `rows` changes nothing: one launch, as ever.  rows = 0 frees the buffer and restores the refusal.
 * mkh_problem_set_sweep_rows itself refuses what mkh_clearance refuses about the checker, rows < 0 (MKH_E_INVALID) and a size
 * that overflows (MKH_E_LIMIT); it synchronizes the device.  Still refused whatever `rows` is, on a checker that has
 * sweep_rows alone: mkh_ladder_refine_free, mkh_solve_trajectory_ladder_free_refined, mkh_select_trajectory_candidates with a
 * checker and mkh_solve_trajectory_multistart_free — what they sweep is produced inside the same call.  They take such a
 * checker through a resource of its own:
 * mkh_problem_set_check_rows(checker, rows) reserves a second device buffer, of `rows` JUDGED rows — a node or a sample judged
 * inside a call, not an interior sample of an edge known in front of it —, one distance (8 bytes) per general convex pair and
 * row, zeroed.  With M = n_samples, mkh_select_trajectory_candidates with a checker and mkh_solve_trajectory_multistart_free
 * need rows >= 1 + M and judge their T * B * S candidate rows in chunks of floor(rows / (1 + M)); mkh_ladder_refine_free and
 * mkh_solve_trajectory_ladder_free_refined need rows >= 1 + 2M AND sweep_rows >= M (the pass sweeps the incoming path, the fused
 * call searches, with sweep_rows) and judge the B loop results of a waypoint step in chunks of floor(rows / (1 + 2M)).  Per
 * chunk a SPECULATIVE pre-pass runs the general convex routine on every row the check could read — its conditions without the
 * node's verdict, which only the check knows: the node itself where it is finite, and the samples of every edge that would be
 * swept behind a free node — and the check reads a subset.  THE RULES do not change and the outputs do not depend on `rows`.
 * check_rows = 0 on such a checker, or a missing sweep_rows where it is needed: MKH_E_INVALID, the message naming what is
 * missing; a positive check_rows below one item: MKH_E_LIMIT.  On a checker without general convex pairs check_rows changes
 * nothing: every call runs the launches it always ran.  rows = 0 frees the buffer.  mkh_problem_set_check_rows itself refuses
 * and returns what mkh_problem_set_sweep_rows does; it synchronizes the device.
 * MKH_E_LIMIT when the poses of a row and the three rows of q beside them (a, b (-) a, q(u)) exceed 64 KB of LDS:
 * 7 nbody + 3 nq > 8192 doubles.  "One call in flight per checker handle" holds as for mkh_clearance.
 */
typedef struct MkhSweptClearanceIO {
  double  *margin;      /* (N,)  required */
  int32_t *sample;      /* (N,)  required */
  int32_t *pair;        /* (N,)  required */
} MkhSweptClearanceIO;
int32_t mkh_swept_clearance(MkhProblem *checker, int32_t N, const double *q_from /* (N, nq) */, const double *q_to /* (N, nq) */,
                            int32_t n_samples, const MkhSweptClearanceIO *io, int32_t flags, void *hip_stream);
int32_t mkh_problem_set_sweep_rows(MkhProblem *checker, int64_t rows /* 0: free the buffer */);
int32_t mkh_problem_set_check_rows(MkhProblem *checker, int64_t rows /* 0: free the buffer */);

/*
 * Certified sweep: a sweep whose sample count follows from how far the edge can move the checker's geoms, and which says whether
 * the SPACE BETWEEN its samples is free as well — "this motion is free", not "these postures are".  A fixed n_samples is too many
 * for a millimetre of wrist correction and far too few for a radian of a shoulder; here every edge gets the count its own motion
 * asks for at a stated resolution, and a lower bound of the clearance over the whole edge.  It builds on THE RULE OF CLEARANCE
 * and THE RULE OF THE SWEEP, whose terms stand unchanged.
 *
 * THE RULE OF THE CERTIFIED SWEEP (mkh_certified_sweep).
 *   The reach table  (mkh_checker_motion_reach) is a model constant of a checker, (n_pairs, njnt, 2) doubles.  For pair k with
 *                  geoms g1, g2 on bodies b1, b2 take the body chains from the world to b1 and to b2 and drop their common prefix:
 *                  joints on common ancestors move both geoms rigidly together and do not change their distance.  For a joint j
 *                  of body c on what remains of the chain of geom g, c = c_0 -> c_1 -> ... -> c_m = body(g):
 *                    coef[k][j][0]  multiplies the joint's LINEAR weight: 1 for a slide or free joint, 0 otherwise.
 *                    coef[k][j][1]  multiplies its ANGULAR weight: 0 for a slide; for a hinge, ball or free joint
 *                                   rho = |jnt_pos_j| + D_after(c, j) + sum_{i=1..m} (|body_pos[c_i]| + D(c_i)) + |geom_pos_g| + r_g.
 *                  D(c) bounds how far body c's own joints move its origin: over its slide joints max(|lo - qpos0|, |hi - qpos0|)
 *                  (+inf for an unlimited slide), plus over its hinge and ball joints 2 |jnt_pos|; +inf for a free joint anywhere
 *                  but as joint j itself.  D_after(c, j) is the same sum over the joints of c behind j.  r_g is the radius of the
 *                  geom about its own centre: sphere r; capsule r + half; ellipsoid max(size); cylinder hypot(r, half); box
 *                  |size|; mesh the largest hull-vertex norm; plane +inf (a plane on the world body has an empty chain: its
 *                  radius is never used).  Joints on neither remaining chain have both coefficients 0.
 *   Edge weights   from the sweep's own b (-) a: hinge rot = |dq|; slide lin = |dq|; ball rot = the angle of the shortest arc;
 *                  free lin = |dp| and rot = the arc's angle.
 *   Motion bound   L_k = sum_j (coef0 lin_j + coef1 rot_j), where a weight of 0 contributes 0 whatever its coefficient (inf * 0
 *                  never occurs); motion = max_k L_k.  The edge is UNBOUNDED when motion is not finite, or when a limited slide
 *                  joint lies outside its range at either end (D presumes the range).
 *   Sample count   M = clamp(ceil(motion / resolution) - 1, 1, max_samples) — one division of doubles —, capped = 1 where the
 *                  unclamped value exceeds max_samples (so an infinite motion is capped); an UNBOUNDED edge has M = max_samples.
 *   Points         u_i = i / (M + 1) for i = 0 .. M + 1, BOTH ends included; q(u_i) by the sweep's blend, unchanged — the ends
 *                  too, so q(u_{M+1}) is a (+) 1 (b (-) a) —; m_{k,i} = (d_k(q(u_i)) - dmin_k) + 0.0 by THE RULE OF CLEARANCE,
 *                  unchanged: the pair list, the ddetect cap, the cull, "a NaN decides".
 *   Outputs        margin = min_i min_k m_{k,i}; sample = the lowest i that attains it; pair = the pair of that point's clearance.
 *                  lower_bound = min over the segments i = 0 .. M and the pairs k of
 *                                1/2 ((m_{k,i} + m_{k,i+1}) - L_k / (M + 1));
 *                  segment and bound_pair attain it, lowest segment first, then lowest pair.  An UNBOUNDED edge has
 *                  lower_bound = -inf, segment = bound_pair = 0.  n_samples = M; motion; capped.
 *                  verdict = 2 (COLLIDES) iff !(margin >= 0); 1 (CERTIFIED FREE) iff margin >= 0 and lower_bound >= 0;
 *                  0 (UNDECIDED) otherwise.
 *   A NaN or an infinity in a or b: margin = lower_bound = motion = NaN; sample = pair = segment = bound_pair = capped = 0;
 *   n_samples = 1; verdict = 2.
 *
 * Why it is a proof.  A point of geom g is carried by joint j at most coef0 lin_j + coef1 rot_j far when the joint alone moves
 * along the edge — a slide by its travel, a rotation about an anchor by the arc, whose lever is at most rho —, and the joints of
 * an edge move in proportion to u; so each geom of pair k moves, relative to the other, at most L_k |du| over a piece du of the
 * edge, and d_k — a distance between the two sets, clamped at ddetect_k or not, a minimum of 1-Lipschitz functions either way —
 * is Lipschitz in u with constant L_k.  Between two neighbouring points, 1 / (M + 1) apart, d_k therefore cannot fall below the
 * crossing point of the two cones that descend from them, which is the expression above.  The clamped distance and the
 * distance ddetect_k of a culled pair are lower bounds of the true one.  So a CERTIFIED edge keeps every pair at or above its dmin
 * for EVERY u in [0, 1], not only at the points.  Certification needs margins at the points of about resolution / 2; the margins
 * of a checker never exceed ddetect - dmin, so a resolution at or above 2 (ddetect - dmin) certifies nothing — edges come out
 * undecided; that is not an error.
 *
 * mkh_certified_sweep evaluates N edges, q_from and q_to (N, nq); all ten outputs are (N,) and required.  Host pointers
 * (synchronous; staged whole) or device pointers with MKH_FLAG_DEVICE_PTRS (asynchronous on the stream); one launch either way,
 * and N is not bound by the checker's max_batch.  The reach table is filled and uploaded at the handle's first such call.
 * MKH_E_INVALID before any device work: resolution not finite or <= 0; max_samples outside [1, 4096]; N < 1; any other flag.  The
 * checker is refused as mkh_clearance refuses it, and in addition: a checker WITH general convex pairs (cylinder-box,
 * ellipsoid-*, mesh hulls) with MKH_E_INVALID, whatever sweep_rows it has — such pairs are not certified yet: sample counts
 * that vary per edge do not fit the chunks of sweep_rows —; MKH_E_LIMIT when a group's slice of LDS — the sweep's, and three rows
 * of n_pairs doubles beside it (L_k, the previous point's margins, this point's distances) — exceeds 64 KB.  "One call in
 * flight per checker handle" holds as for mkh_clearance.
 * mkh_checker_motion_reach writes the (n_pairs, njnt, 2) reach table to host memory; it needs no device work and serves any
 * checker with collision pairs.
 */
typedef struct MkhCertifiedSweepIO {
  double  *margin;       /* (N,)  every field required */
  int32_t *sample;       /* (N,)  0 .. n_samples + 1 */
  int32_t *pair;         /* (N,) */
  double  *lower_bound;  /* (N,) */
  int32_t *segment;      /* (N,)  0 .. n_samples */
  int32_t *bound_pair;   /* (N,) */
  int32_t *n_samples;    /* (N,) */
  double  *motion;       /* (N,) */
  int32_t *capped;       /* (N,) */
  int32_t *verdict;      /* (N,)  MKH_SWEEP_* */
} MkhCertifiedSweepIO;
#define MKH_SWEEP_UNDECIDED 0
#define MKH_SWEEP_CERTIFIED 1
#define MKH_SWEEP_COLLIDES  2
int32_t mkh_certified_sweep(MkhProblem *checker, int32_t N, const double *q_from /* (N, nq) */, const double *q_to /* (N, nq) */,
                            double resolution, int32_t max_samples, const MkhCertifiedSweepIO *io, int32_t flags, void *hip_stream);
int32_t mkh_checker_motion_reach(MkhProblem *checker, double *out /* (n_pairs, njnt, 2), host memory */);

/*
 * Ladder-graph trajectory IK: S IK solutions per waypoint (a "rung"), computed independently of each other, and a dynamic
 * program over the T rungs that picks the path — complete first, free of joint-space jumps second, shortest third.  It is the
 * per-waypoint search ACROSS candidates that mkh_solve_trajectory_multistart leaves out: that call keeps one whole candidate,
 * this one may change branch at every waypoint.  No counterpart in the reference.
 *
 * THE RULE (mkh_ladder_select; mkh_solve_trajectory_ladder runs it on the rungs it solves).
 * Nodes.  Instance b, waypoint t, node s: configurations q_nodes (B, T, S, nq) and flags tracked (B, T, S), a node counting as
 * tracked when its flag is != 0.  1 <= S <= 256 (back-pointers are bytes) and 1 <= T <= 65 535 (the two counts of a key are 16
 * bits each); beyond either: MKH_E_LIMIT.
 *
 * Edge cost.  For t >= 1, from node s of rung t - 1 to node s' of rung t:
 *   d = sum_k w_k ((q_{t,s'} (-) q_{t-1,s})_k)^2   multi-start's distance, the same device function: (-) = mj_differentiatePos at
 *                                                   dt = 1, w = weights (nv,), each >= 0, or ones when NULL
 *   c = d when 0 <= d <= DBL_MAX, else +inf         (a NaN or an overflow in either node: an edge nobody prefers)
 * The START EDGE of node (0, s) is c(q_{0,s}, q[b]), from the caller's current posture q (B, nq) — the convention of
 * mkh_solve_trajectory_multistart's length.  An edge with t >= 1 is a BREAK when c > max_step_sq; max_step_sq >= 0, +inf: nothing is
 * ever a break; NaN or negative: MKH_E_INVALID.  The start edge is never a break.
 *
 * Key of a path (one node per rung), compared lexicographically:
 *   lost    = its nodes with tracked == 0
 *   breaks  = its break edges
 *   length  = the sum of its c, start edge included, accumulated in ascending t by one rounded addition each — never fused
 *             into the products inside d.  inf + x = inf: no NaN can arise.
 *
 * Recurrence.
 *   K[0][s']  = (lost(0, s'), 0, c_start(s'))
 *   K[t][s']  = min over s of  K[t-1][s] + (lost(t, s'), break(s -> s'), c(s -> s')),   pred[t][s'] = the LOWEST s attaining it
 *   end node  = the lowest s with minimal K[T-1][s];  the path is the back-trace through pred.
 * Rounded addition is monotone, so the recurrence is well defined; THE RESULT IS DEFINED BY THE RECURRENCE, not by "the optimum
 * over the real numbers": a restatement that performs the same additions in the same order reproduces it.
 *
 * Outputs, per instance: node_index (B, T) the chosen s per waypoint; n_tracked (B,) = T - lost; n_breaks (B,); path_length
 * (B,); edge_break (B, T): 1 where the edge INTO waypoint t is a break, entry 0 always 0.  Optional gather through the path:
 * q_path[b, t] = q_nodes[b, t, node_index[b, t]].  Everything runs on the device, one wavefront per instance, without atomics;
 * the back-pointers and break bits live in a workspace of the handle of B·T·(S + 8·ceil(S / 64)) bytes.
 *
 * Pointers are host pointers (staged, synchronous) or device pointers with MKH_FLAG_DEVICE_PTRS (asynchronous on the stream).
 * A model for which one tile of 64 destination nodes, the keys, the joint table, the weights and one source node exceed 64 KB of
 * LDS (nq beyond about 115): MKH_E_LIMIT.
 */
typedef struct MkhLadderIO {
  int32_t *node_index;      /* (B, T)      the chosen node per waypoint                                           required  */
  int32_t *n_tracked;       /* (B,)        tracked nodes on the path                                              required  */
  int32_t *n_breaks;        /* (B,)        break edges on the path                                                required  */
  double *path_length;      /* (B,)        its length                                                             required  */
  int32_t *edge_break;      /* (B, T)      1 where the edge into waypoint t is a break                            required  */
  double *q_path;           /* (B, T, nq)  optional: q_nodes gathered through the path                                      */
} MkhLadderIO;
int32_t mkh_ladder_select(MkhProblem *problem, int32_t B, int32_t T, int32_t S, const double *q, const double *q_nodes,
                          const int32_t *tracked, const double *weights, double max_step_sq, const MkhLadderIO *io,
                          int32_t flags, void *hip_stream);

/*
 * THE RULE, with a checker (mkh_ladder_select_free; mkh_solve_trajectory_ladder_free runs it on the rungs it solves): the path
 * whose waypoints AND motions are free of collision.  The checker is an ARGUMENT of these calls; a checker attached with
 * mkh_problem_set_collision_check is neither read nor needed here (mkh_ladder_select_free ignores one;
 * mkh_solve_trajectory_ladder_free refuses one, as every ladder call that runs loops does).
 *   Nodes.   node_margin(t, s) = the margin of q_{t,s} by THE RULE OF CLEARANCE.  The EFFECTIVE flag of a node is
 *            tracked(t, s) != 0 && node_margin(t, s) >= 0: a node in collision counts as not tracked.
 *   Edges.   For t >= 1, blocked(t, s', s) = the edge from node (t - 1, s) to node (t, s') COLLIDES by THE RULE OF THE SWEEP
 *            with M = n_samples.  An edge whose DESTINATION node is not tracked by the effective flag is not swept — its
 *            waypoint is lost on any path through it —: its swept margin is NaN and blocked = 0.  The start edge from q[b] is
 *            never swept, just as it is never a break.
 *   Key.     Only the first component changes.  Waypoint t of a path counts as LOST when its node is not tracked by the
 *            effective flag, or — for t >= 1 — the edge into it collides.  In the recurrence the term lost(t, s') becomes
 *            lost(t, s') | blocked(t, s', s); breaks, length, the tie order (lowest s, lowest end node), the 16-bit counts and
 *            the back-trace are unchanged.  n_tracked = T - lost therefore counts the waypoints that are reached, tracked,
 *            free of collision and entered by a free motion.
 *   Outputs, beside MkhLadderIO's: edge_collision (B, T): 1 where the edge INTO waypoint t collides, entry 0 always 0;
 *            n_edge_collisions (B,); edge_margin (B, T): the swept margin of the chosen edge, entry 0 = +inf, NaN where the edge
 *            was not swept.  Optional: node_margin (B, T, S); edge_margin_all (B, T, S, S), entry [b, t, s', s], NaN for t = 0
 *            and for edges not swept.
 * The full mask is the defined result: every edge into an effectively tracked node is swept, B (T - 1) S^2 M row evaluations
 * at the most, into one flag byte per edge in a workspace of the PROBLEM handle (B T S^2 bytes; B T S^2 doubles more only when
 * edge_margin_all is asked for); the node clearances run on the checker handle.  The checker must pass mkh_swept_clearance's
 * refusals and live on the problem's device and belong to its MkhModel (MKH_E_INVALID); n_samples >= 1; B T S^2 < 2^31.
 * "One call in flight per checker handle" holds.
 */
typedef struct MkhLadderFreeIO {
  int32_t *edge_collision;     /* (B, T)        1 where the edge into waypoint t collides                          required  */
  int32_t *n_edge_collisions;  /* (B,)          colliding edges on the path                                        required  */
  double *edge_margin;         /* (B, T)        the swept margin of the chosen edges                               required  */
  double *node_margin;         /* (B, T, S)     optional: the clearance margin of every node                                 */
  double *edge_margin_all;     /* (B, T, S, S)  optional: the swept margin of every edge                                     */
} MkhLadderFreeIO;
int32_t mkh_ladder_select_free(MkhProblem *problem, MkhProblem *checker, int32_t B, int32_t T, int32_t S, const double *q,
                               const double *q_nodes, const int32_t *tracked, const double *weights, double max_step_sq,
                               int32_t n_samples, const MkhLadderIO *io, const MkhLadderFreeIO *free_io, int32_t flags,
                               void *hip_stream);

/*
 * THE RULE, with a certifying checker (mkh_ladder_select_certified; mkh_solve_trajectory_ladder_certified runs it on the rungs it
 * solves): THE RULE "with a checker" above with ONE term replaced — how an edge is judged.  Nodes, the effective flag, the key,
 * the ties, the breaks, the 16-bit counts and the back-trace are that rule's, unchanged; so is the gating: the destination must be
 * effectively tracked, the start edge from q[b] is never swept, an edge that is not swept has NaN margins and is not blocked.
 *   Edges.   For t >= 1 the edge from node (t - 1, s) to an effectively tracked node (t, s') is judged by THE RULE OF THE
 *            CERTIFIED SWEEP, unchanged, on (q_{t-1,s}, q_{t,s'}) at the call's `resolution` and `max_samples`: BOTH ends are
 *            points of the edge, as that rule has them, and the sample count follows from the edge's own motion bound.  margin,
 *            lower_bound, n_samples and verdict of a swept edge are BITWISE what mkh_certified_sweep returns for that pair of rows.
 *   blocked(t, s', s) follows `edge_policy`:
 *            MKH_EDGE_REJECT_COLLIDING  (0)  blocked iff verdict == MKH_SWEEP_COLLIDES: the sampled rule's reading, at the
 *                                            points the motion bound asks for.
 *            MKH_EDGE_REQUIRE_CERTIFIED (1)  blocked iff verdict != MKH_SWEEP_CERTIFIED: an UNDECIDED edge is blocked as well, so
 *                                            every waypoint n_tracked counts is entered by a motion PROVEN free for every u.
 *            Any other value: MKH_E_INVALID.
 *   What differs from the sampled rule, beside the count: the end points are judged.  The destination of a swept edge is free
 *            by the gating, but its SOURCE may be a colliding node: the sampled rule looks at interior samples only and may call
 *            such an edge free; here it COLLIDES, so the waypoint behind a colliding node is lost on that path as well.
 *   Outputs. MkhLadderIO's and MkhLadderFreeIO's keep their meaning — edge_collision and n_edge_collisions are "what the search
 *            counted as blocked on the chosen path": under MKH_EDGE_REQUIRE_CERTIFIED that INCLUDES the undecided edges —;
 *            edge_margin (B, T) is the certified sweep's margin of the chosen edge, both ends included; edge_margin_all as there.
 *            MkhLadderCertifiedIO adds, of the chosen path: edge_verdict (B, T) MKH_SWEEP_*, -1 where the edge was not swept
 *            (t = 0 included); edge_lower_bound (B, T), +inf at t = 0, NaN where not swept; edge_n_samples (B, T), 0 where not
 *            swept; n_certified (B,) = the t >= 1 on the path with verdict MKH_SWEEP_CERTIFIED.  Optional: edge_verdict_all
 *            (B, T, S, S) int8, entry [b, t, s', s], -1 for t = 0 and for edges not swept.
 * One launch judges every edge into an effectively tracked node, a second one the chosen edges; the mask lives where the
 * sampled rule's does, B T S^2 bytes more only when edge_verdict_all is asked for, and B T doubles and 2 B T int32 for the path's
 * new outputs of a host-pointer call.  Refused before any device work: everything mkh_ladder_select_free refuses; resolution not
 * finite or <= 0, max_samples outside [1, 4096], an edge_policy other than the two (MKH_E_INVALID); the checker as
 * mkh_certified_sweep refuses it — general convex pairs with MKH_E_INVALID whatever its sweep_rows, its LDS slice beyond 64 KB
 * with MKH_E_LIMIT.  The reach table is filled and uploaded at the checker's first such call.  Refinement
 * (mkh_ladder_refine_free) and candidate tracking (mkh_select_trajectory_candidates) still sample: they judge rows inside
 * their own kernels.
 */
#define MKH_EDGE_REJECT_COLLIDING  0
#define MKH_EDGE_REQUIRE_CERTIFIED 1
typedef struct MkhLadderCertifiedIO {
  int32_t *edge_verdict;       /* (B, T)        MKH_SWEEP_* of the chosen edges, -1: not swept                      required  */
  double *edge_lower_bound;    /* (B, T)        the certified sweep's lower bound of the chosen edges              required  */
  int32_t *edge_n_samples;     /* (B, T)        their sample counts, 0: not swept                                  required  */
  int32_t *n_certified;        /* (B,)          chosen edges proven free                                           required  */
  int8_t *edge_verdict_all;    /* (B, T, S, S)  optional: the verdict of every edge                                          */
} MkhLadderCertifiedIO;
int32_t mkh_ladder_select_certified(MkhProblem *problem, MkhProblem *checker, int32_t B, int32_t T, int32_t S, const double *q,
                                    const double *q_nodes, const int32_t *tracked, const double *weights, double max_step_sq,
                                    double resolution, int32_t max_samples, int32_t edge_policy, const MkhLadderIO *io,
                                    const MkhLadderFreeIO *free_io, const MkhLadderCertifiedIO *certified_io, int32_t flags,
                                    void *hip_stream);

/*
 * mkh_solve_trajectory_ladder: the rungs solved by multi-start, then THE RULE above.
 *
 * Rungs.  Rung t of instance b is what mkh_solve_multistart returns in q_all / converged_all / status_all / iters_all for
 * target row (target_index0 + b)·T + t of the flattened (B·T) targets, BITWISE: the same seeding rule and generator
 * u(rng_seed, (target_index0 + b)·T + t, s, k); seed 0 of every rung is the caller's q[b]; io->seeds (B, T, S, nq) as the
 * alternative (row 0 of every rung is still replaced by q[b]); an attached seed table is queried with every waypoint's OWN
 * frame targets, S - 1 nearest.  The B·T·S loops do not depend on each other: they run as one multi-start launch, or in chunks
 * of whole rungs when B·T·S > max_batch (S <= max_batch is needed).  Node (b, t, s) is TRACKED when its loop converged and its
 * status carries no bit but MKH_ST_OUTSIDE_LIMITS.
 *
 * Targets.  frame_targets (B, T, n_frame, 7).  posture_target is shared by the whole call — (n_posture, nq) — or, with
 * MKH_FLAG_POSTURE_BATCHED, (B, T, n_posture, nq); the same for com_target with MKH_FLAG_COM_BATCHED.  Threshold mode only
 * (both thresholds >= 0), at least one frame task, no dense rows.  MKH_FLAG_WARM_START does not enter, as in multi-start.
 *
 * Outputs.  The search's, and the chosen nodes' rows q_traj, v_traj, status, iters, converged in (B, T, .).  Optional: qvel by
 * mkh_solve_trajectory's rule on the chosen path with q_{-1} = q; q_all (B, T, S, nq), v_all, status_all, iters_all,
 * converged_all (B, T, S): every node; seeds_out (B, T, S, nq): the starts.  Pointers follow the call's convention; every
 * argument error is reported before any device work.
 */
typedef struct MkhTrajectoryLadderIO {
  const double *seeds;      /* (B, T, S, nq) caller-defined starts, or NULL: drawn, or from the attached seed table          */
  const double *weights;    /* (nv,) weights of the edge cost, each >= 0, or NULL: ones                                      */
  double max_step_sq;       /* the break gate on the edge cost, >= 0; +inf: no gate                                          */
  double *q_traj;           /* (B, T, nq)  the chosen nodes' configurations                                        required  */
  double *v_traj;           /* (B, T, nv)  their last velocities                                                   required  */
  int32_t *status;          /* (B, T)      their MKH_ST_* bits                                                     required  */
  int32_t *iters;           /* (B, T)      their iteration counts                                                  required  */
  int32_t *converged;       /* (B, T)      their loops' converged flags                                            required  */
  int32_t *node_index;      /* (B, T)      as MkhLadderIO                                                          required  */
  int32_t *n_tracked;       /* (B,)                                                                                required  */
  int32_t *n_breaks;        /* (B,)                                                                                required  */
  double *path_length;      /* (B,)                                                                                required  */
  int32_t *edge_break;      /* (B, T)                                                                              required  */
  double *qvel;             /* (B, T, nv)  optional: (q_t (-) q_{t-1}) / waypoint_dt along the path, q_{-1} = q              */
  double *seeds_out;        /* (B, T, S, nq) optional: the starts the loops ran from                                         */
  double *q_all;            /* (B, T, S, nq) optional: every node's configuration                                            */
  double *v_all;            /* (B, T, S, nv) optional                                                                        */
  int32_t *status_all;      /* (B, T, S)   optional                                                                          */
  int32_t *iters_all;       /* (B, T, S)   optional                                                                          */
  int32_t *converged_all;   /* (B, T, S)   optional                                                                          */
  double waypoint_dt;       /* > 0 when qvel is given                                                                        */
} MkhTrajectoryLadderIO;
int32_t mkh_solve_trajectory_ladder(MkhProblem *problem, int32_t B, int32_t T, int32_t n_seeds, const double *q,
                                    const double *frame_targets, const double *posture_target, const double *com_target,
                                    double dt, double damping, int32_t max_iters, double pos_threshold, double ori_threshold,
                                    uint64_t rng_seed, int64_t target_index0, const MkhTrajectoryLadderIO *io, int32_t flags,
                                    void *hip_stream);

/*
 * Ladder refinement: a pass AFTER the search that re-tracks the chosen path across its breaks and lost nodes.  The rungs of a
 * ladder are solved independently of each other, so consecutive chosen nodes may sit on different IK branches and the search
 * can only choose among what the rungs hold; the pass re-solves the offending waypoints from their neighbours on the path.  It
 * works on the B chosen paths only and costs 2T - 1 loop launches on B instances: about two plain trajectory calls.
 *
 * THE RULE OF THE REFINEMENT (mkh_ladder_refine; mkh_solve_trajectory_ladder_refined runs it on the path it searched).  The
 * terms are those of THE RULE above: the edge cost c(a -> b) = sum_k w_k ((b (-) a)_k)^2 with its +inf for a NaN or an overflow,
 * the same device function; the gate max_step_sq (>= 0, +inf legal: then only lost nodes are repaired); the start edge from
 * q[b], which is never a break; the key (lost, breaks, length), length accumulated in ascending t by one rounded addition each.
 *
 * Input, per instance b: a path p_0 ... p_{T-1}, q_path (B, T, nq); flags tracked_path (B, T), != 0: tracked; the waypoint
 * targets of mkh_solve_trajectory_ladder, in its shapes; the loop parameters dt, damping, max_iters, pos_threshold >= 0,
 * ori_threshold >= 0.  A loop result TRACKS when its loop converged and its status carries no bit but MKH_ST_OUTSIDE_LIMITS —
 * the ladder's own definition.
 *
 * Working path r, initialised to p.  Two sweeps; every waypoint of a sweep is ONE launch of mkh_solve_until's loop on all B
 * instances with waypoint t's targets, stream-ordered, no host synchronisation in between.
 *  1. Forward, t = 0 ... T-1, with r_{-1} = q[b].  Waypoint t of instance b is BAD when r_t is not tracked, or when t >= 1 and
 *     c(r_{t-1} -> r_t) > max_step_sq.  The launch starts bad instances at r_{t-1}, all others at r_t (their result is discarded;
 *     a converged posture ends its loop after one step).  A bad instance's result x is ACCEPTED when it tracks and, for t >= 1,
 *     c(r_{t-1} -> x) <= max_step_sq.  Accepted: r_t = x, r_t counts as tracked, repaired[b, t] = 1, and v, status, iters,
 *     converged of (b, t) become the loop's.  Otherwise nothing of (b, t) changes.
 *  2. Backward, t = T-2 ... 0.  Waypoint t is bad when r_t is not tracked or c(r_t -> r_{t+1}) > max_step_sq; bad instances
 *     start at r_{t+1}; x is accepted when it tracks and c(x -> r_{t+1}) <= max_step_sq; then repaired[b, t] = 2.  An accepted
 *     repair may turn the edge INTO t into a break: that edge is judged at t - 1, the next step of the sweep; the start edge
 *     stays exempt.  T = 1: the sweep is empty.
 *  3. Guard.  The key of r and the key of p are computed by one device function, which also yields edge_break, n_tracked,
 *     n_breaks and path_length of whichever path is returned.  r is returned only if its key is STRICTLY smaller,
 *     lexicographically; then refined[b] = 1.  Otherwise every output of instance b is the input path's, bit for bit,
 *     repaired[b, :] = 0 and refined[b] = 0.  THE RESULT IS NEVER WORSE THAN THE PATH THAT CAME IN — than the search's, in the
 *     composed call.
 *
 * Threshold mode only, at least one frame task, no dense rows; MKH_FLAG_WARM_START does not enter, as in multi-start.  B <=
 * max_batch.  The working path, the loops' rows of the repaired nodes, the start array and the flags live in the handle's
 * workspace: about B·T·((2 nq + nv)·8 + 24) bytes.
 *
 * mkh_ladder_refine: the pass alone.  Outputs: q_path_out (B, T, nq) the returned path; tracked_out (B, T) its 0 / 1 flags;
 * repaired (B, T): 0 kept, 1 / 2 replaced by the forward / backward sweep; refined (B,); edge_break, n_tracked, n_breaks,
 * path_length of the returned path.  Optional v, status, iters, converged (B, T, .): the loops' rows of the REPAIRED nodes of a
 * returned r; rows of kept nodes are left unwritten, so a caller pre-fills them with what it knows of its path.  q_path_out may
 * be q_path itself, tracked_out may be tracked_path.  Pointers are host pointers (staged, synchronous; v ... converged are
 * then copied in, updated and copied back) or device pointers with MKH_FLAG_DEVICE_PTRS (asynchronous on the stream).  Every
 * argument error is reported before any device work.
 */
typedef struct MkhLadderRefineIO {
  const double *weights;    /* (nv,) weights of the edge cost, each >= 0, or NULL: ones                                      */
  double max_step_sq;       /* the break gate on the edge cost, >= 0; +inf: no gate                                          */
  double *q_path_out;       /* (B, T, nq)  the returned path                                                       required  */
  int32_t *tracked_out;     /* (B, T)      its tracked flags                                                       required  */
  int32_t *repaired;        /* (B, T)      0 kept, 1 forward sweep, 2 backward sweep                               required  */
  int32_t *refined;         /* (B,)        1 where the working path was returned                                   required  */
  int32_t *edge_break;      /* (B, T)      1 where the edge into waypoint t of the returned path is a break        required  */
  int32_t *n_tracked;       /* (B,)                                                                                required  */
  int32_t *n_breaks;        /* (B,)                                                                                required  */
  double *path_length;      /* (B,)                                                                                required  */
  double *v;                /* (B, T, nv)  optional: rows of repaired nodes only                                             */
  int32_t *status;          /* (B, T)      optional: the same                                                                */
  int32_t *iters;           /* (B, T)      optional: the same                                                                */
  int32_t *converged;       /* (B, T)      optional: the same                                                                */
} MkhLadderRefineIO;
int32_t mkh_ladder_refine(MkhProblem *problem, int32_t B, int32_t T, const double *q, const double *q_path,
                          const int32_t *tracked_path, const double *frame_targets, const double *posture_target,
                          const double *com_target, double dt, double damping, int32_t max_iters, double pos_threshold,
                          double ori_threshold, const MkhLadderRefineIO *io, int32_t flags, void *hip_stream);

/*
 * THE RULE OF THE REFINEMENT, with a checker (mkh_ladder_refine_free; mkh_solve_trajectory_ladder_free_refined runs it on the path
 * it searched): the pass above whose repairs are checked as nodes and whose motions are swept.  The terms are those of THE RULE OF
 * THE REFINEMENT, of THE RULE "with a checker" and of THE RULE OF THE SWEEP, unchanged; only what follows is amended.  The checker
 * is an ARGUMENT, M = n_samples >= 1.
 *   State of a path (the input path p and the working path r alike).  node_margin(t) by THE RULE OF CLEARANCE.  The EFFECTIVE
 *     flag of waypoint t is tracked(t) != 0 && node_margin(t) >= 0.  For t >= 1, edge_margin(t) is the swept margin of the edge
 *     INTO t with M samples; that edge is swept iff its DESTINATION is effectively tracked, whatever its source is — otherwise its
 *     margin is NaN and it does not collide.  The start edge from q[b] is never swept: its margin is +inf.  An edge COLLIDES iff
 *     it was swept and !(margin >= 0).
 *   Initial state of r = that of p: one clearance of the B·T rows of p on the checker handle (in chunks of its max_batch, as
 *     mkh_ladder_select_free's nodes) and one sweep of the path's edges — p seen as a ladder of width 1.
 *   Forward, waypoint t.  BAD when r_t is not effectively tracked, or — t >= 1 — c(r_{t-1} -> r_t) > max_step_sq, or — t >= 1 —
 *     the edge into t collides.  Bad instances start at r_{t-1} (q[b] for t = 0), as before.  The result x of a bad instance is
 *     ACCEPTED when it tracks, margin(x) >= 0 and, for t >= 1, c(r_{t-1} -> x) <= max_step_sq and the swept edge r_{t-1} -> x does
 *     not collide.  Accepted: r_t = x, effectively tracked, repaired = 1, the loop's rows are taken, as before; node_margin(t) =
 *     margin(x); edge_margin(t) = that sweep's margin (t = 0: +inf stays); and for t + 1 < T edge_margin(t+1) is evaluated anew
 *     for the edge x -> r_{t+1} — swept iff r_{t+1} is effectively tracked, else NaN.  Otherwise nothing of (b, t) changes.
 *   Backward, t = T-2 ... 0.  BAD when r_t is not effectively tracked, or c(r_t -> r_{t+1}) > max_step_sq, or the edge into t + 1
 *     collides.  Bad instances start at r_{t+1}.  x is accepted when it tracks, margin(x) >= 0, c(x -> r_{t+1}) <= max_step_sq
 *     and the edge x -> r_{t+1} does not collide (it is swept iff r_{t+1} is effectively tracked).  Accepted: repaired = 2;
 *     edge_margin(t+1) = that sweep's margin; for t >= 1 edge_margin(t) is evaluated anew for r_{t-1} -> x — its destination x is
 *     tracked, so it is always swept.  That edge is judged at t - 1, the next step, exactly as a new break is.
 *   Guard.  The key is the checked ladder's: waypoint t counts as LOST when it is not effectively tracked, or — t >= 1 — the edge
 *     into it collides; breaks and length are unchanged.  r is returned only on a strictly smaller key; otherwise every output is
 *     the input path's, bit for bit.  tracked_out holds the EFFECTIVE flags of the returned path: a kept node that collides comes
 *     back with 0.  New outputs, of the returned path: node_margin (B, T); edge_margin (B, T), entry 0 = +inf, NaN where the edge
 *     was not swept; edge_collision (B, T), entry 0 = 0; n_edge_collisions (B,).  n_tracked = T - lost counts the waypoints that
 *     are tracked, free, and entered by a free motion.
 *   NaN.  "A NaN decides", as in the two rules used: a candidate with a NaN row is in collision and is never accepted.
 * The checks run on the device between the loop launch of a waypoint and the kernel that commits it: per bad instance whose x
 * tracks at most 2M + 1 rows — margin(x); the edge the acceptance judges; the edge the commit would create — built in LDS, only
 * three margins per instance (and per block its samples are dealt to) written; a colliding x skips its edges.  No host synchronisation between steps.
 *
 * mkh_ladder_refine_free: mkh_ladder_refine's arguments, refusals and pointer conventions, with the checker, n_samples and the
 * new outputs.  The checker is refused as mkh_ladder_select_free refuses it (general convex pairs, another model, another device;
 * n_samples < 1); a checker ATTACHED to the problem is refused as before.  "One call in flight per checker handle" holds.
 */
typedef struct MkhLadderRefineFreeIO {
  int32_t *edge_collision;     /* (B, T)  1 where the edge into waypoint t of the returned path collides         required  */
  int32_t *n_edge_collisions;  /* (B,)    colliding edges on the returned path                                  required  */
  double *edge_margin;         /* (B, T)  the swept margins of its edges                                        required  */
  double *node_margin;         /* (B, T)  optional: the clearance margins of its nodes                                    */
} MkhLadderRefineFreeIO;
int32_t mkh_ladder_refine_free(MkhProblem *problem, MkhProblem *checker, int32_t B, int32_t T, const double *q,
                               const double *q_path, const int32_t *tracked_path, const double *frame_targets,
                               const double *posture_target, const double *com_target, double dt, double damping,
                               int32_t max_iters, double pos_threshold, double ori_threshold, int32_t n_samples,
                               const MkhLadderRefineIO *io, const MkhLadderRefineFreeIO *free_io, int32_t flags,
                               void *hip_stream);

/*
 * mkh_solve_trajectory_ladder_refined: mkh_solve_trajectory_ladder and, with `refine` != NULL, the pass above on the path it
 * searched — the rungs, the search, the gathers and the pass on the device, nothing over the bus in between.  The result is
 * BITWISE mkh_solve_trajectory_ladder followed by mkh_ladder_refine on its outputs (q_traj and the chosen nodes' tracked flags
 * as the path, v_traj ... converged pre-filled).  The returned path goes where the ladder's goes — io's q_traj, v_traj, status,
 * iters, converged, n_tracked, n_breaks, path_length, edge_break —, the gate and the weights are io's, and of `refine` only
 * tracked_out, repaired and refined are used (required); its other fields are ignored.  qvel, when asked for, follows the
 * returned path.  node_index keeps the search's choice: at a repaired waypoint it names the node that was replaced.  With
 * refine == NULL the call IS mkh_solve_trajectory_ladder, which is a wrapper around it.
 */
int32_t mkh_solve_trajectory_ladder_refined(MkhProblem *problem, int32_t B, int32_t T, int32_t n_seeds, const double *q,
                                            const double *frame_targets, const double *posture_target,
                                            const double *com_target, double dt, double damping, int32_t max_iters,
                                            double pos_threshold, double ori_threshold, uint64_t rng_seed,
                                            int64_t target_index0, const MkhTrajectoryLadderIO *io,
                                            const MkhLadderRefineIO *refine, int32_t flags, void *hip_stream);

/*
 * mkh_solve_trajectory_ladder_nodes: the ladder on K = n_nodes DEDUPLICATED nodes per rung.  The S = n_seeds loop results of a
 * rung are reduced to at most K distinct ones by THE RULE OF THE SET on the device, between the loops and the search; the
 * search then runs on (B, T, K) nodes.  The search costs T·K² instead of T·S², the node workspace holds B·T·K rows instead of
 * B·T·S, and S is no longer bounded by the search's 256 (back-pointers are bytes) but by the set's 4 096 candidates.
 *
 * THE RULE, for rung (b, t):
 *   The candidates are the S loop results, BITWISE what mkh_solve_multistart gives in q_all / converged_all / status_all /
 *   iters_all for target row (target_index0 + b)·T + t — seeding, io->seeds, an attached seed table exactly as in
 *   mkh_solve_trajectory_ladder.
 *   With MKH_FLAG_UNWIND_TURNS they are unwound toward q[b] (THE RULE OF THE UNWINDING); their flags are carried over.
 *   THE RULE OF THE SET runs on them with K = n_nodes, r = min_distance, q_ref = q[b] and the ladder's weights (io->weights);
 *   a candidate is eligible when it is TRACKED in the ladder's sense (converged, no status bit but MKH_ST_OUTSIDE_LIMITS) —
 *   which is the set's own eligibility.
 *   Node (b, t, j) is slot j of that set; it is tracked iff j < n_distinct.  An empty slot holds candidate 0's row, as the
 *   set rule says, and is not tracked.
 *   THE RULE of the ladder then runs on the (B, T, K) nodes, unchanged: node_index (B, T) is a SLOT index in 0 .. K-1.
 *   The refinement, with `refine` != NULL, runs on the chosen path, unchanged (as in mkh_solve_trajectory_ladder_refined; of
 *   `refine` only tracked_out, repaired and refined are used).
 * The nodes of a rung are a subset of its S candidates (up to the unwinding), so the path's key is never smaller than the
 * plain ladder's on the same loops, and n_tracked is EQUAL: a rung holds a tracked node iff it holds a tracked candidate.
 * With n_nodes >= n_seeds, min_distance = 0 and the flag clear, the nodes of a rung are its tracked candidates in ascending
 * d_ref (bitwise copies merged), and on every instance WHOSE RUNGS ALL HOLD A TRACKED CANDIDATE (n_tracked == T) the chosen
 * path's q_traj, n_breaks and path_length are the plain ladder's, ties between equal keys aside.  On a rung nobody tracked the
 * plain ladder chooses among S untracked rows, this call holds candidate 0's row only: there the key may be larger.
 *
 * Limits.  1 <= n_nodes <= 64 (the set's; the search's 256 lies above it); 1 <= n_seeds <= 4 096, n_seeds <= max_batch;
 * min_distance >= 0 and finite; T, max_step_sq, the targets, the thresholds and the weights as in mkh_solve_trajectory_ladder.
 * Every argument error is reported before any device work.
 *
 * Workspace.  The loops of a chunk (whole rungs, at most max_batch loops) write into multi-start's candidate buffers of ONE
 * chunk; the selection writes the chunk's slots straight into the (B·T, K, .) node arrays.  Nothing the call allocates is
 * sized B·T·S; only io->seeds and io->seeds_out, when the caller passes them, have that size (a host caller's are staged
 * whole, like every input and output of a host-pointer call).
 *
 * Outputs.  `io` is mkh_solve_trajectory_ladder's struct: the chosen nodes' rows, the search's outputs, qvel — and its optional
 * q_all (B, T, K, nq), v_all (B, T, K, nv), status_all, iters_all, converged_all (B, T, K) are the NODES' rows (converged_all
 * of an empty slot is candidate 0's flag); seeds_out (B, T, S, nq) stays the starts.  `nodes` holds what is new, all required:
 * node_seed_index, node_multiplicity, node_distance (B, T, K) — the slots' seed_index (-1: empty), multiplicity and d_ref of the
 * set rule; n_distinct, n_converged, n_uncovered (B, T) — the set rule's per-target counts; seed_index (B, T) — the chosen
 * node's candidate index s (-1 where the chosen slot is empty: a lost waypoint).
 */
typedef struct MkhLadderNodesIO {
  int32_t *node_seed_index;    /* (B, T, K)  the candidate each node is; -1: empty slot                           required  */
  int32_t *node_multiplicity;  /* (B, T, K)  candidates the node covers; 0: empty slot                            required  */
  double *node_distance;       /* (B, T, K)  its d_ref to q[b]; +inf: empty slot                                  required  */
  int32_t *n_distinct;         /* (B, T)     nodes filled                                                         required  */
  int32_t *n_converged;        /* (B, T)     tracked candidates                                                   required  */
  int32_t *n_uncovered;        /* (B, T)     tracked candidates no node covers                                    required  */
  int32_t *seed_index;         /* (B, T)     the chosen node's candidate index                                    required  */
} MkhLadderNodesIO;
int32_t mkh_solve_trajectory_ladder_nodes(MkhProblem *problem, int32_t B, int32_t T, int32_t n_seeds, int32_t n_nodes,
                                          double min_distance, const double *q, const double *frame_targets,
                                          const double *posture_target, const double *com_target, double dt, double damping,
                                          int32_t max_iters, double pos_threshold, double ori_threshold, uint64_t rng_seed,
                                          int64_t target_index0, const MkhTrajectoryLadderIO *io, const MkhLadderNodesIO *nodes,
                                          const MkhLadderRefineIO *refine, int32_t flags, void *hip_stream);

/*
 * mkh_solve_trajectory_ladder_free: the ladder calls above with THE RULE "with a checker" in place of THE RULE.  The arguments
 * are those of the call on distinct nodes, with the checker, n_samples and the MkhLadderFreeIO: n_nodes = 0 with nodes = NULL is
 * mkh_solve_trajectory_ladder on n_seeds nodes per rung, n_nodes = K >= 1 with nodes the ladder on K distinct nodes (anything
 * else: MKH_E_INVALID).  `refine` must be NULL here: the checked pass is mkh_solve_trajectory_ladder_free_refined's, below.
 *   Behind the loops of every chunk of rungs the clearance of the candidates' final q runs on the checker and
 *   MKH_ST_IN_COLLISION is OR-ed into their status rows — status_all in the plain ladder; the chunk's candidate rows in the call
 *   on nodes, behind the optional unwinding and in front of the selection, so that a colliding candidate takes no slot and a
 *   FILLED slot's status never carries the bit (an empty slot holds candidate 0's rows, as in the plain call, and is not tracked).  A node's tracked flag follows from its status as before, so a colliding node is not
 *   tracked: that IS the effective flag of the rule.  Then the sweep of every edge into a tracked node, the masked search, and
 *   everything behind it as in the plain calls.
 * The result is the composition of the plain call's nodes (return_all), the clearance of those rows, and mkh_ladder_select_free
 * on them, bit for bit.  free_io->node_margin must be NULL here (the nodes' verdict is the status bit); edge_margin_all is
 * (B, T, W, W) with W the nodes per rung.  The checker is an argument: a checker ATTACHED to the problem is refused as in the
 * plain calls.  Checker refusals, n_samples and sizes as in mkh_ladder_select_free.
 */
int32_t mkh_solve_trajectory_ladder_free(MkhProblem *problem, MkhProblem *checker, int32_t B, int32_t T, int32_t n_seeds,
                                         int32_t n_nodes, double min_distance, const double *q, const double *frame_targets,
                                         const double *posture_target, const double *com_target, double dt, double damping,
                                         int32_t max_iters, double pos_threshold, double ori_threshold, uint64_t rng_seed,
                                         int64_t target_index0, int32_t n_samples, const MkhTrajectoryLadderIO *io,
                                         const MkhLadderNodesIO *nodes, const MkhLadderRefineIO *refine,
                                         const MkhLadderFreeIO *free_io, int32_t flags, void *hip_stream);

/*
 * mkh_solve_trajectory_ladder_free_refined: mkh_solve_trajectory_ladder_free's arguments with `refine` REQUIRED (of it only
 * tracked_out, repaired and refined are used, as in the plain refined calls).  The result is BITWISE
 * mkh_solve_trajectory_ladder_free followed by mkh_ladder_refine_free on its outputs: q_traj as the path, the chosen nodes'
 * effective flags as its flags, v_traj ... converged pre-filled.  The returned path goes where the ladder's goes; free_io's
 * edge_collision, n_edge_collisions and edge_margin follow the returned path (edge_margin_all stays the search's; node_margin
 * must be NULL as above); qvel follows the returned path; node_index keeps the search's choice.  n_nodes = 0 and n_nodes = K
 * as in mkh_solve_trajectory_ladder_free, which keeps refusing a `refine` of its own.
 */
int32_t mkh_solve_trajectory_ladder_free_refined(MkhProblem *problem, MkhProblem *checker, int32_t B, int32_t T, int32_t n_seeds,
                                                 int32_t n_nodes, double min_distance, const double *q,
                                                 const double *frame_targets, const double *posture_target,
                                                 const double *com_target, double dt, double damping, int32_t max_iters,
                                                 double pos_threshold, double ori_threshold, uint64_t rng_seed,
                                                 int64_t target_index0, int32_t n_samples, const MkhTrajectoryLadderIO *io,
                                                 const MkhLadderNodesIO *nodes, const MkhLadderRefineIO *refine,
                                                 const MkhLadderFreeIO *free_io, int32_t flags, void *hip_stream);

/*
 * mkh_solve_trajectory_ladder_certified: mkh_solve_trajectory_ladder_free with THE RULE "with a certifying checker" in place of
 * THE RULE "with a checker": its arguments with n_samples replaced by resolution, max_samples and edge_policy, and the
 * MkhLadderCertifiedIO behind the MkhLadderFreeIO.  n_nodes = 0 with nodes = NULL is the plain ladder, n_nodes = K >= 1 with nodes
 * the ladder on K distinct nodes, as there; everything in front of the edges — the loops, the clearance of the candidates, the
 * status bit, the nodes' flags — is that call's.  The result is the composition of the plain call's nodes (return_all), the
 * clearance of those rows, and mkh_ladder_select_certified on them, bit for bit.  `refine` must be NULL: the refinement pass
 * still samples, and a path judged by two rules is nobody's result.  free_io->node_margin must be NULL as there;
 * edge_margin_all and edge_verdict_all are (B, T, W, W) with W the nodes per rung.  Refusals as in
 * mkh_solve_trajectory_ladder_free and mkh_ladder_select_certified.
 */
int32_t mkh_solve_trajectory_ladder_certified(MkhProblem *problem, MkhProblem *checker, int32_t B, int32_t T, int32_t n_seeds,
                                              int32_t n_nodes, double min_distance, const double *q, const double *frame_targets,
                                              const double *posture_target, const double *com_target, double dt, double damping,
                                              int32_t max_iters, double pos_threshold, double ori_threshold, uint64_t rng_seed,
                                              int64_t target_index0, double resolution, int32_t max_samples, int32_t edge_policy,
                                              const MkhTrajectoryLadderIO *io, const MkhLadderNodesIO *nodes,
                                              const MkhLadderRefineIO *refine, const MkhLadderFreeIO *free_io,
                                              const MkhLadderCertifiedIO *certified_io, int32_t flags, void *hip_stream);

/* Same inputs; additionally writes the requested intermediates (build_ik / compute_error /
 * compute_jacobian / get_transform_frame_to_world parity taps).  v_out/status_out may be NULL
 * to skip the QP. */
int32_t mkh_eval(MkhProblem *problem, int32_t B, const double *q, const double *frame_targets,
                 const double *posture_target, const double *com_target, double dt, double damping,
                 double *v_out, int32_t *status_out, const MkhTaps *taps, int32_t flags, void *hip_stream);

/* Configuration.integrate (mink/configuration.py:214-226): q_out[b] = q[b] (+) v[b]*dt. */
int32_t mkh_integrate(MkhModel *model, int32_t B, const double *q, const double *v, double dt,
                      double *q_out, int32_t flags, void *hip_stream);

/*
 * The SO3/SE3 device functions of the hot path (mkh lie_dev.h), evaluated element-wise over n inputs — the
 * same code the frame-task lanes run, exposed so that it can be held directly against the reference's
 * known-answer vectors (mink/lie/so3.py, mink/lie/se3.py, mink/lie/base.py:107-156).  Poses are wxyz_xyz (7),
 * rotations wxyz (4), tangents (v, ω) (6); matrices row-major.  `b` may be NULL for unary ops.
 *   MKH_LIE_SE3_LOG      a (n,7)          -> out (n,6)    SE3.log            se3.py:159-185
 *   MKH_LIE_SE3_JLOG     a (n,7)          -> out (n,36)   jlog = rjacinv(log) base.py:150-156
 *   MKH_LIE_SE3_LJACINV  a (n,6)          -> out (n,36)   SE3.ljacinv        se3.py:210-218
 *   MKH_LIE_SE3_MULTIPLY a (n,7), b (n,7) -> out (n,7)    a @ b              se3.py:144-151
 *   MKH_LIE_SE3_INVERSE  a (n,7)          -> out (n,7)    se3.py:136-142
 *   MKH_LIE_SE3_RMINUS   a (n,7), b (n,7) -> out (n,6)    a.rminus(b) = log(b^-1 a)  base.py:111-112
 *   MKH_LIE_SO3_LOG      a (n,4)          -> out (n,3)    SO3.log            so3.py:176-191
 *   MKH_LIE_SO3_MATRIX   a (n,4)          -> out (n,9)    SO3.as_matrix      so3.py:111-114
 *   MKH_LIE_SE3_APPLY    a (n,7), b (n,3) -> out (n,3)    SE3.apply          se3.py:153-157
 */
#define MKH_LIE_SE3_LOG 0
#define MKH_LIE_SE3_JLOG 1
#define MKH_LIE_SE3_LJACINV 2
#define MKH_LIE_SE3_MULTIPLY 3
#define MKH_LIE_SE3_INVERSE 4
#define MKH_LIE_SE3_RMINUS 5
#define MKH_LIE_SO3_LOG 6
#define MKH_LIE_SO3_MATRIX 7
#define MKH_LIE_SE3_APPLY 8
int32_t mkh_lie_eval(int32_t device, int32_t op, int32_t n, const double *a, const double *b, double *out,
                     int32_t flags, void *hip_stream);

/* mujoco.mj_geomDistance(model, data, geom1, geom2, distmax, fromto) — the third-party routine behind every row of
 * CollisionAvoidanceLimit (mink/limits/collision_avoidance_limit.py:214-229) — element-wise on the device routines of the
 * collision phase (primitive geoms; parity tests only, host pointers).  pairs (n, 22): per pair two records of
 * (mjtGeom type, size[3], world position[3], world quaternion wxyz[4]); dist_out (n): the signed distance, distmax when
 * nothing is closer, NaN for a pair of types without a routine; fromto_out (n, 6): the connecting segment, geom1 → geom2. */
int32_t mkh_geom_distance_eval(int32_t device, int32_t n, const double *pairs, double distmax, double *dist_out,
                               double *fromto_out, void *hip_stream);

/* Launch geometry of the most recent solve / eval on this problem (the kernel variant depends on the call; see
 * mkh_problem_last_kernel); before any launch, that of the lean direct variant for a batch of B.  For benchmarks
 * and occupancy reports. */
int32_t mkh_problem_launch_info(const MkhProblem *problem, int32_t B, int32_t *grid, int32_t *block,
                                int32_t *lds_bytes, int32_t *tableau_rows);

#ifdef __cplusplus
}
#endif
#endif /* MINKHIP_H_ */
