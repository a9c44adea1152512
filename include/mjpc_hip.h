/*
 * mjpc_hip.h — C ABI of the MI355X-native Predictive-Sampling rollout engine.
 *
 * This is the drop-in boundary for ONE path of hartikainen/mujoco_mpc:
 *   mjpc/planners/sampling/planner.cc:342-380  (SamplingPlanner::Rollouts, the ThreadPool fan-out)
 *   mjpc/trajectory.cc:100-210                 (Trajectory::NoisyRollout, the horizon loop)
 *   mjpc/trajectory.cc:312-326                 (Trajectory::UpdateReturn)
 *   mjpc/planners/sampling/planner.cc:168-181  (partial_sort -> winner)
 *
 * Plain C, plain pointers and sizes, no C++/torch types.  Every array is fp64
 * (mjtNum == double in the reference) or int32.
 *
 * MjpcHipModel mirrors the fields of MuJoCo's `mjModel` the path reads (same names, same
 * layout, same units) so that the reference-side shim is a field-by-field pointer copy
 * from the `mjModel*` handed to `SamplingPlanner::Initialize`
 * (mjpc/planners/sampling/planner.cc:40-76).  See INTEGRATION.md.
 */
#ifndef MJPC_HIP_H_
#define MJPC_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- enums (numeric values identical to MuJoCo 3.1.4 / MJPC) ------------------------- */
enum { MJPC_JNT_FREE = 0, MJPC_JNT_BALL = 1, MJPC_JNT_SLIDE = 2, MJPC_JNT_HINGE = 3 };
enum {
  MJPC_GEOM_PLANE = 0, MJPC_GEOM_HFIELD = 1, MJPC_GEOM_SPHERE = 2, MJPC_GEOM_CAPSULE = 3,
  MJPC_GEOM_ELLIPSOID = 4, MJPC_GEOM_CYLINDER = 5, MJPC_GEOM_BOX = 6, MJPC_GEOM_MESH = 7
};
enum { MJPC_CONE_PYRAMIDAL = 0, MJPC_CONE_ELLIPTIC = 1 };
enum { MJPC_SOL_NEWTON = 2, MJPC_INT_EULER = 0, MJPC_INT_IMPLICIT = 2, MJPC_INT_IMPLICITFAST = 3 };
/* model features outside this view (MjpcHipModel.unsupported) */
enum { MJPC_EQ_CONNECT = 0, MJPC_EQ_WELD = 1, MJPC_EQ_JOINT = 2, MJPC_EQ_TENDON = 3 };      /* mjtEq */
enum { MJPC_DYN_NONE = 0, MJPC_DYN_INTEGRATOR = 1, MJPC_DYN_FILTER = 2, MJPC_DYN_FILTEREXACT = 3 };   /* mjtDyn */
enum { MJPC_UNSUP_FLUID = 1,          /* fluid forces of the ellipsoid model (a geom with fluidshape="ellipsoid") */
       MJPC_UNSUP_GRAVCOMP = 2,       /* (no longer set: body_gravcomp travels in the view) */
       MJPC_UNSUP_ACTUATOR_GAIN = 4,  /* gaintype other than fixed, biastype other than none / affine */
       MJPC_UNSUP_ACTUATOR_DYN = 8,   /* dyntype muscle / user, actnum != 1, actearly */
       MJPC_UNSUP_SPATIAL_TENDON = 16,/* wrap objects other than joints */
       MJPC_UNSUP_JNT_ACTFRC = 32,    /* (no longer set: jnt_actfrclimited / jnt_actfrcrange travel in the view) */
       MJPC_UNSUP_FLEX_SKIN_PLUGIN = 64 /* flexes, plugins, user callbacks other than the residual */ };
enum { MJPC_DSBL_CONSTRAINT = 1 << 0, MJPC_DSBL_EQUALITY = 1 << 1, MJPC_DSBL_FRICTIONLOSS = 1 << 2, MJPC_DSBL_LIMIT = 1 << 3,
       MJPC_DSBL_SENSOR = 1 << 12, MJPC_DSBL_MIDPHASE = 1 << 13, MJPC_ENBL_OVERRIDE = 1 << 0, MJPC_ENBL_MULTICCD = 1 << 4 };
enum { MJPC_DSBL_CONTACT = 1 << 4 };            /* mjDSBL_CONTACT */
enum { MJPC_BIAS_NONE = 0, MJPC_BIAS_AFFINE = 1 };
/* spline interpolation, mjpc/spline/spline.h:30-34 */
enum { MJPC_SPLINE_ZERO = 0, MJPC_SPLINE_LINEAR = 1, MJPC_SPLINE_CUBIC = 2 };
/* norm types, mjpc/norm.h:27-38 */
enum {
  MJPC_NORM_NULL = -1, MJPC_NORM_QUADRATIC = 0, MJPC_NORM_L22 = 1, MJPC_NORM_L2 = 2,
  MJPC_NORM_COSH = 3, MJPC_NORM_POWER = 5, MJPC_NORM_SMOOTHABS = 6, MJPC_NORM_SMOOTHABS2 = 7,
  MJPC_NORM_RECTIFY = 8
};
/* built-in device residuals (the reference dispatches through the global mjcb_sensor
 * callback, mjpc/app.cc:110-126; a GPU cannot call back into host C++) */
enum {
  MJPC_TASK_PARTICLE = 0,   /* mjpc/test/testdata/particle_residual.h:33-43 */
  MJPC_TASK_CARTPOLE = 1,   /* mjpc/tasks/cartpole/cartpole.cc:36-49 */
  MJPC_TASK_QUADRUPED = 2,  /* mjpc/tasks/quadruped/quadruped.cc:33-221 */
  MJPC_TASK_COPYSTATE = 3,  /* residual = [qpos,qvel] (mjpc/test/agent/rollout_test.cc:40-60) */
  MJPC_TASK_HUMANOID_TRACK = 4, /* mjpc/tasks/humanoid/tracking/tracking.cc:94-216 */
  MJPC_TASK_HUMANOID_STAND = 5, /* mjpc/tasks/humanoid/stand/stand.cc:41-94 */
  MJPC_TASK_HUMANOID_WALK = 6,  /* mjpc/tasks/humanoid/walk/walk.cc:44-166 */
  MJPC_TASK_SHADOW_REORIENT = 7, /* mjpc/tasks/shadow_reorient/hand.cc:37-84; int_data = [palm site, cube body, goal body, key] */
  MJPC_TASK_WALKER = 8,     /* mjpc/tasks/walker/walker.cc:39-57; int_data = [torso body]; parameters = [height goal, speed goal] */
  MJPC_TASK_ACROBOT = 9,    /* mjpc/tasks/acrobot/acrobot.cc:34-49; int_data = [goal site, tip site] */
  MJPC_TASK_QUADRUPED_HILL = 10, /* mjpc/tasks/quadruped/quadruped.cc:726-768; int_data = [trunk body, sites FR FL RR RL, stage];
                                 * dbl_data = the stage goals [nstage][7] (mpos, mquat of task_hill.xml:82-101) for the host Transition */
  MJPC_TASK_PARTICLE_TIMEVARYING = 11, /* mjpc/tasks/particle/particle.cc:30-50 ("Particle"): tip position - Lissajous goal of data->time,
                                 * tip velocity, control (6 residuals); int_data = [tip site] */
  MJPC_TASK_PARTICLE_FIXED = 12, /* particle.cc:68-73 ("ParticleFixed"): the same with goal = mocap_pos[0..1] */
  MJPC_TASK_SWIMMER = 14,        /* mjpc/tasks/swimmer/swimmer.cc:33-46: control (nu), nose - target in the plane (2); int_data = [nose geom, targets reached] */
  MJPC_TASK_HUMANOID_INTERACT = 15, /* mjpc/tasks/humanoid/interact/interact.cc:31-186: int_data = [body torso, pelvis, foot_right, foot_left, head,
                                  * shin_right, shin_left, has facing target, (body1, body2) x 5 (-1: pair not selected)]; dbl_data = [facing target
                                  * x, y, (local_pos1[3], local_pos2[3]) x 5]; parameters = [head height goal, torso height goal] */
  MJPC_TASK_FINGERS = 16,        /* mjpc/tasks/fingers/fingers.cc:31-62: finger_a - object, finger_b - object (framepos of the bodies), distance of the three
                                  * object sites to their targets, control; int_data = [body finger_a, finger_b, object, sites 0 1 2, sites 0t 1t 2t] */
  MJPC_TASK_QUADROTOR = 13,      /* mjpc/tasks/quadrotor/quadrotor.cc:37-60: position - goal, linear / angular velocity, control - hover thrust (13 of
                                 * the 15 declared residuals are written); int_data = [body, stage]; dbl_data = stage goals [nstage][7] */
  MJPC_TASK_ALLEGRO = 17,        /* mjpc/tasks/allegro/allegro.cc:36-77: the Shadow residual with 16-wide slices (57 residuals); int_data = [grasp site,
                                  * cube body, goal body, key] */
  MJPC_TASK_OP3 = 18,            /* mjpc/tasks/op3/stand.cc:34-152 (53 residuals, rows by mode): int_data = [mode (0 Stand, 1 Handstand), sites head,
                                  * left_foot, right_foot, left_hand, right_hand, torso, body body_link]; parameters = [height goal] */
  MJPC_TASK_TABLE = 19           /* the caller's own residual, described by a table in int_data / dbl_data (below): no device code per task */
};
/* ---- MJPC_TASK_TABLE: a residual as a table --------------------------------------------------------------------------------
 * The residual is a list of BLOCKS.  Block b writes `dim` consecutive rows starting at `row`; the blocks cover [0, num_residual)
 * exactly once, in ascending order.  A block is a sum of TERMS,  v[k] = sum_j coef_j * src_j[off_j + k],  added in table order,
 * followed by one operation:
 *   MJPC_TBL_OP_SUM      rows = v[0 .. dim)  (ncomp = dim; a block without terms writes zeros)
 *   MJPC_TBL_OP_NORM     one row (dim = 1): sqrt(sum_{k < ncomp} v[k]^2), 1 <= ncomp <= MJPC_TBL_MAX_NORM, at least one term
 *   MJPC_TBL_OP_SUBQUAT  three rows (dim = 3, ncomp = 4), exactly two terms, both quaternions (MJPC_TBL_QUAT or MJPC_TBL_MOCAP_QUAT,
 *                        off = 0): coef_0 * mju_subQuat(src_0, src_1); coef_1 is not read
 * A SOURCE is a vector; a term reads `ncomp` components of it from its offset `off` on (xy of a position: off 0 of a 2-row block;
 * its z: off 2 of a 1-row block; a slice of qpos: off = first index):
 *   kind                          components  id             reads
 *   MJPC_TBL_CONST                objtype     first index    dbl_data[id .. id + objtype)  (the record's objtype field holds the count)
 *   MJPC_TBL_PARAM                num_parameter  -           MjpcHipTask.parameters (mjpc_hip_set_task moves a goal without a new table)
 *   MJPC_TBL_QPOS / QVEL / ACT    nq / nv / na   -           the candidate's state at this step (ACT: refused when na = 0; qpos as the
 *                                                            position stage leaves it: free / ball joint quaternions normalised)
 *   MJPC_TBL_CTRL / ACTUATOR_FORCE  nu           -           the step's control / actuator forces
 *   MJPC_TBL_KEY_QPOS             nq          key            key_qpos[key]
 *   MJPC_TBL_MOCAP_POS / QUAT / MAT  3 / 4 / 9  mocap body   the plan input's mocap pose as handed in (MAT: the quaternion's matrix, row-major)
 *   MJPC_TBL_SUBTREE_COM / LINVEL 3           body           centre of mass of the body's subtree / its linear velocity
 *   MJPC_TBL_POS / QUAT / MAT     3 / 4 / 9   object         frame of the object `objtype` = MJPC_OBJ_BODY (the body's INERTIAL frame, as
 *   MJPC_TBL_XAXIS / YAXIS / ZAXIS  3         object         MuJoCo's objtype="body" sensors read it), MJPC_OBJ_XBODY (the body's own frame),
 *   MJPC_TBL_LINVEL / ANGVEL      3           object         MJPC_OBJ_GEOM or MJPC_OBJ_SITE, in the world frame: what the framepos / framequat /
 *                                                            frame?axis / framelinvel / frameangvel sensors give (MAT row-major; a quaternion
 *                                                            of a site / geom / inertial frame is xquat[body] * the local quaternion)
 * The sources above are position- and velocity-stage quantities: the residual runs beside the constraint solve.  The time is not a
 * source.  Accelerations and contact forces are LATE sources, evaluated after the solve by the one-step calls only:
 *   MJPC_TBL_QACC                 nv          -              qacc of the converged solve (after the noslip pass where the model has one):
 *                                                            the acceleration mj_forward reports, not the integrator's damped one
 *   MJPC_TBL_LINACC / ANGACC      3           object         world-frame linear / angular acceleration of the object's frame (objtype as for
 *                                                            LINVEL), as framelinacc / frameangacc: the linear one carries -gravity (a body at
 *                                                            rest reads +9.81 z) and the omega x v term of a moving point
 *   MJPC_TBL_ACCELEROMETER        3           site           LINACC of the site in the site's frame (objtype = MJPC_OBJ_SITE)
 *   MJPC_TBL_GYRO / VELOCIMETER   3           site           ANGVEL / LINVEL of the site in the site's frame (objtype = MJPC_OBJ_SITE)
 *   MJPC_TBL_TOUCH                1           site           objtype = the zone's shape MJPC_ZONE_*, off = index into dbl_data of the zone's
 *                                                            size[3] (MuJoCo's size conventions; the component offset is 0): the sum of the
 *                                                            normal forces of the contacts that took part in the solve, have a geom on the
 *                                                            site's body, a positive normal force and their position p (site coordinates)
 *                                                            inside the zone: sphere |p| <= r; box |p_i| <= s_i; ellipsoid sum (p_i / s_i)^2
 *                                                            <= 1; cylinder p_x^2 + p_y^2 <= r^2 and |p_z| <= h; capsule: distance to the
 *                                                            segment +-h z at most r.  Normal force: the first row's force (frictionless /
 *                                                            elliptic), the sum of the 2 (dim - 1) edge forces (pyramidal).  (MuJoCo also
 *                                                            counts a contact outside the zone whose normal ray crosses it: not done here.)
 * Late rules.  A block with a late term is a LATE BLOCK: its other terms may only be late kinds, CONST or PARAM, and its operation is
 * SUM or NORM.  TOUCH names a site, a known shape, positive sizes and a dbl_data range in bounds; ACCELEROMETER / GYRO / VELOCIMETER
 * name a site.  Late rows exist in the one-step calls only (mjpc_hip_step_batch, mjpc_hip_transition_fd, mjpc_hip_linearize_step,
 * mjpc_hip_unscented_moments and what is built on them).  In a rollout (mjpc_hip_plan*) late rows are written as 0.0: the cost term
 * that covers them should carry weight 0 (the reference's estimator sensors sit outside the cost as well).  Sums run in ascending
 * dof index and ascending contact index.
 * Encoding.  int_data = [MJPC_TBL_VERSION, nblock, nterm,  nblock x {op, row, dim, ncomp, first term, number of terms},
 *                        nterm x {kind, objtype (CONST: count; 0 where the kind has none), id (0 where the kind has none), off}];
 * a block's terms are consecutive and the blocks use the terms in order.  dbl_data = [coef_0 .. coef_{nterm-1}, constants ...].
 * Caps: nblock <= MJPC_TBL_MAX_BLOCKS, nterm <= MJPC_TBL_MAX_TERMS.  mjpc_hip_create / mjpc_hip_layout_bytes / mjpc_hip_set_task
 * refuse a table that breaks any rule above or names an object, key, mocap body, parameter or dbl_data index out of range;
 * mjpc_hip_last_error names the block and term.  mjpc_hip_set_task may install another table of at most the created size.
 * Example, the Walker task (control, torso height - goal, torso z axis z - 1, forward speed - goal; torso = body 1, nu = 6):
 *   int_data = {1, 4, 7,   SUM,0,6,6,0,1,  SUM,6,1,1,1,2,  SUM,7,1,1,3,2,  SUM,8,1,1,5,2,
 *               CTRL,0,0,0,   POS,MJPC_OBJ_XBODY,1,2,  PARAM,0,0,0,   ZAXIS,MJPC_OBJ_XBODY,1,2,  CONST,1,7,0,
 *               SUBTREE_LINVEL,0,1,0,  PARAM,0,0,1}
 *   dbl_data = {1, 1, -1, 1, -1, 1, -1,   1.0}            parameters = {height goal, speed goal} */
enum { MJPC_TBL_OP_SUM = 0, MJPC_TBL_OP_NORM = 1, MJPC_TBL_OP_SUBQUAT = 2 };
enum { MJPC_TBL_CONST = 0, MJPC_TBL_PARAM = 1, MJPC_TBL_QPOS = 2, MJPC_TBL_QVEL = 3, MJPC_TBL_ACT = 4, MJPC_TBL_CTRL = 5,
       MJPC_TBL_ACTUATOR_FORCE = 6, MJPC_TBL_KEY_QPOS = 7, MJPC_TBL_MOCAP_POS = 8, MJPC_TBL_MOCAP_QUAT = 9, MJPC_TBL_MOCAP_MAT = 10,
       MJPC_TBL_SUBTREE_COM = 11, MJPC_TBL_SUBTREE_LINVEL = 12, MJPC_TBL_POS = 13, MJPC_TBL_QUAT = 14, MJPC_TBL_MAT = 15,
       MJPC_TBL_XAXIS = 16, MJPC_TBL_YAXIS = 17, MJPC_TBL_ZAXIS = 18, MJPC_TBL_LINVEL = 19, MJPC_TBL_ANGVEL = 20,
       /* late kinds (one-step calls only) */
       MJPC_TBL_QACC = 21, MJPC_TBL_LINACC = 22, MJPC_TBL_ANGACC = 23, MJPC_TBL_ACCELEROMETER = 24, MJPC_TBL_GYRO = 25,
       MJPC_TBL_VELOCIMETER = 26, MJPC_TBL_TOUCH = 27 };
enum { MJPC_ZONE_SPHERE = 2, MJPC_ZONE_CAPSULE = 3, MJPC_ZONE_ELLIPSOID = 4, MJPC_ZONE_CYLINDER = 5, MJPC_ZONE_BOX = 6 };   /* mjtGeom values */
#define MJPC_TBL_VERSION 1
#define MJPC_TBL_MAX_BLOCKS 64
#define MJPC_TBL_MAX_TERMS 256
#define MJPC_TBL_MAX_NORM 16
enum { MJPC_TRN_JOINT = 0, MJPC_TRN_TENDON = 3, MJPC_TRN_SITE = 4 };   /* mjtTrn values of the supported actuator transmissions */
enum { MJPC_OBJ_BODY = 1, MJPC_OBJ_XBODY = 2, MJPC_OBJ_GEOM = 5, MJPC_OBJ_SITE = 6 };

/* failure[] bits: why a candidate's rollout stopped (any bit => total_return = MJPC_MAX_RETURN, like
 * CheckWarnings -> failure, mjpc/utilities.cc:787-799 + trajectory.cc:169-173) */
enum {
  MJPC_WARN_BADQPOS = 1, MJPC_WARN_BADQVEL = 2, MJPC_WARN_BADQACC = 4,   /* mjWARN_BADQPOS / BADQVEL / BADQACC */
  MJPC_WARN_CONTACTFULL = 8, MJPC_WARN_CNSTRFULL = 16,                    /* mjWARN_CONTACTFULL / CNSTRFULL (nconmax / nefcmax) */
  MJPC_WARN_RAY = 32,                                                     /* Ground() ray hit nothing (utilities.cc:549-552) */
  MJPC_WARN_SYNC = 64,                                                    /* engine-internal: a wave hand-shake timed out */
  MJPC_WARN_UNSUPPORTED = 128   /* a geom pair without a collider came within reach of contact (none left among the pairs create() accepts) */
};
#define MJPC_MINVAL 1e-15           /* mjMINVAL */
#define MJPC_MAX_RETURN 1.0e6       /* kMaxReturnValue, mjpc/trajectory.cc:29 */
#define MJPC_MAX_COST_TERMS 128     /* kMaxCostTerms, mjpc/task.h */
#define MJPC_MAX_HORIZON 512        /* kMaxTrajectoryHorizon, mjpc/trajectory.h:27 */

/* ---- model: the subset of mjModel the path reads ------------------------------------- */
/* ABI revision of this header.  mjpc_hip_version() returns the revision the library was built from; both view structs start
   with `struct_size` (= sizeof of the struct as the CALLER compiled it): mjpc_hip_create / mjpc_hip_set_task / mjpc_hip_layout_bytes refuse a view
   whose size differs from the library's, so a stale .so paired with a newer header (or ctypes layout) fails loudly instead of reading
   garbage pointers.  Bindings without the header: mjpc_hip_sizeof_model() / _task() / _plan_input() / _plan_output(). */
#define MJPC_HIP_ABI_VERSION 4

typedef struct MjpcHipModel {
  int struct_size;                  /* sizeof(MjpcHipModel) */
  /* sizes */
  int nq, nv, nu, na, nbody, njnt, ngeom, nsite, nmocap, nuserdata, nkey, nexclude, ntendon, nwrap, nmesh, nmeshvert, nhfield, nhfielddata;
  /* mjOption */
  double timestep;
  double gravity[3];
  double impratio;
  double tolerance;        /* solver tolerance (1e-8) */
  double ls_tolerance;     /* line-search tolerance (0.01) */
  int cone;                /* MJPC_CONE_* */
  int iterations;          /* max Newton iterations (100) */
  int ls_iterations;       /* max line-search iterations (50) */
  int disableflags;        /* mjDSBL_* bits: constraint, frictionloss, limit, contact are honoured; equality / sensor / midphase have
                            * nothing to act on; any other bit (passive, gravity, clampctrl, warmstart, filterparent, actuation,
                            * refsafe, eulerdamp) is refused at create */
  int enableflags;         /* mjENBL_* bits: override and multiccd are refused, the rest has nothing to act on */
  int solver;              /* mjtSolver: only MJPC_SOL_NEWTON (2, MuJoCo's default and what every MJPC task uses) */
  int integrator;          /* mjtIntegrator: MJPC_INT_EULER (0; with implicit joint damping, mj_Euler), MJPC_INT_IMPLICITFAST (3: also implicit in
                            * tendon damping, the velocity terms of affine actuator biases - zero while the force sits on its forcerange - and
                            * the inertia-box fluid forces; no Coriolis derivative; symmetric factorisation) or MJPC_INT_IMPLICIT (2: the same
                            * plus the velocity derivative of the bias forces, mjd_rne_vel, and an LU factorisation of the non-symmetric
                            * M - h dF/dv).  RK4 is refused */
  int noslip_iterations;   /* mjOption.noslip_iterations: > 0 runs mj_solNoSlip after the Newton solve (friction-loss rows and the friction
                            * dimensions of the contacts re-solved without regularisation; noslip_tolerance at the end of this struct) */
  int neq;                 /* number of equality constraints (eq_* below): connect, weld, joint and (fixed-)tendon equalities; flex is refused */
  int unsupported;         /* MJPC_UNSUP_* bits found by whoever fills this view in parts of mjModel the view does not carry
                            * (integration/hip_sampling_planner.cc: FillModelView); non-zero is refused at create */
  /* mjStatistic */
  double meaninertia;
  /* fluid forces of the inertia-box model (mj_passive): medium density / viscosity and wind (mjOption); all zero = none.  With the
   * implicitfast integrator they are refused (their velocity derivative is not implemented); the ellipsoid model (geom fluidshape)
   * is MJPC_UNSUP_FLUID */
  double density, viscosity, wind[3];
  /* engine capacities (0 = default); overflow => candidate failure, like MuJoCo's
   * "contact/constraint buffer full" warnings -> mjpc CheckWarnings (utilities.cc:787-799) */
  int nconmax, nefcmax;
  /* bodies */
  const int *body_parentid, *body_rootid, *body_weldid, *body_mocapid;
  const int *body_jntnum, *body_jntadr, *body_dofnum, *body_dofadr;
  const double *body_pos, *body_quat, *body_ipos, *body_iquat;
  const double *body_mass, *body_subtreemass, *body_inertia, *body_invweight0;
  /* joint-level clamp of the total actuator force on a hinge / slide joint (mjModel.jnt_actfrclimited / jnt_actfrcrange, applied to
   * qfrc_actuator at the end of mj_fwdActuation); NULL = none */
  const int *jnt_actfrclimited; const double *jnt_actfrcrange;
  const double *body_gravcomp;      /* [nbody] gravity compensation (mj_passive: force -gravity * mass * gravcomp at the body's com), NULL = none */
  /* joints */
  const int *jnt_type, *jnt_qposadr, *jnt_dofadr, *jnt_bodyid, *jnt_limited;
  const double *jnt_pos, *jnt_axis, *jnt_stiffness, *jnt_range, *jnt_margin;
  const double *jnt_solref, *jnt_solimp;      /* limit solver params: 2 / 5 per joint */
  const double *qpos0, *qpos_spring;
  /* dofs */
  const int *dof_bodyid, *dof_jntid, *dof_parentid;
  const double *dof_armature, *dof_damping, *dof_frictionloss, *dof_invweight0;
  const double *dof_solref, *dof_solimp;      /* friction-loss solver params */
  /* geoms */
  const int *geom_type, *geom_contype, *geom_conaffinity, *geom_condim, *geom_bodyid;
  const int *geom_group, *geom_priority;
  const double *geom_size, *geom_pos, *geom_quat, *geom_friction, *geom_solmix;
  const double *geom_solref, *geom_solimp, *geom_margin, *geom_gap, *geom_rbound;
  /* <contact><exclude>: (body1 << 16) + body2, as mjModel.exclude_signature */
  const int *exclude_signature;
  /* equality constraints [neq] (mj_instantiateEquality): MJPC_EQ_CONNECT obj = the two bodies (obj2 may be the world 0), eq_data[0..2]
   * / [3..5] = the anchor in either body frame; MJPC_EQ_WELD obj = the two bodies, eq_data[0..2] = anchor in body 2, [3..5] = the same point in
   * body 1, [6..9] = quaternion of body 2 in body 1's frame (mj_setConst has filled both), [10] = torquescale; MJPC_EQ_JOINT obj = joint1 and joint2 (or -1), eq_data[0..4] = polycoef of
   * q1 - q1_0 = poly(q2 - q2_0); MJPC_EQ_TENDON the same with the lengths of two fixed tendons (relative to their length at qpos0).  eq_active0 = 0 rows are left out (no run-time activation).  All NULL when neq = 0 */
  const int *eq_type, *eq_obj1id, *eq_obj2id, *eq_active0;
  const double *eq_data;            /* 11 per equality (mjNEQDATA) */
  const double *eq_solref, *eq_solimp;   /* 2 / 5 per equality */
  /* sites */
  const int *site_bodyid;
  const double *site_pos, *site_quat;
  /* actuators (joint or fixed-tendon transmission; gain fixed; bias none/affine: motor, general, position servos) */
  const int *actuator_trntype;      /* MJPC_TRN_JOINT / MJPC_TRN_TENDON / MJPC_TRN_SITE (without a reference site: the wrench actuator_gear6 in the
                                     * site frame, motors only - biastype none; with one: actuator_refsite at the end of this struct) */
  const int *actuator_trnid;        /* joint, tendon or site id (first of the 2 mjModel ints) */
  const int *actuator_ctrllimited, *actuator_forcelimited, *actuator_biastype;
  const double *actuator_gainprm;   /* 3 per actuator (first 3 of mjNGAIN) */
  const double *actuator_biasprm;   /* 3 per actuator (first 3 of mjNBIAS) */
  const double *actuator_gear;      /* 1 per actuator (first of 6) */
  const double *actuator_gear6;     /* 6 per actuator (mjModel.actuator_gear as it is): read for site transmissions only; may be NULL without them */
  const double *actuator_ctrlrange, *actuator_forcerange;
  /* activation states (na > 0): one state per stateful actuator (actnum 1).  dyntype MJPC_DYN_*: integrator act_dot = ctrl; filter /
   * filterexact act_dot = (ctrl - act) / max(mjMINVAL, dynprm[0]); the force of a stateful actuator is gain * act + bias.  Euler
   * advance act += h * act_dot (filterexact: act_dot * tau * (1 - exp(-h / tau))), clamped to actrange when actlimited.  All NULL
   * (na = 0): no stateful actuator.  Muscles, user dynamics and actearly are MJPC_UNSUP_ACTUATOR_DYN. */
  const int *actuator_dyntype, *actuator_actadr, *actuator_actlimited;
  const double *actuator_dynprm;    /* 1 per actuator (first of mjNDYN): the time constant */
  const double *actuator_actrange;  /* 2 per actuator */
  /* fixed tendons (wrap objects are joints; wrap_prm = coefficient) */
  const int *tendon_adr, *tendon_num, *tendon_limited, *wrap_objid;
  const double *wrap_prm, *tendon_range, *tendon_margin, *tendon_solref_lim, *tendon_solimp_lim, *tendon_invweight0;
  /* passive tendon forces (mj_passive): spring with a dead band [lengthspring[2t], lengthspring[2t+1]], damper; [ntendon] each,
   * NULL = none.  tendon_frictionloss > 0 makes a friction-loss row along the tendon (mjCNSTR_FRICTION_TENDON) with the solver
   * parameters tendon_solref_fri [2 per tendon] / tendon_solimp_fri [5 per tendon] (NULL = MuJoCo's defaults). */
  const double *tendon_stiffness, *tendon_damping, *tendon_lengthspring, *tendon_frictionloss;
  const double *tendon_solref_fri, *tendon_solimp_fri;
  /* convex meshes (collision = convex hull of the vertices, in the geom frame; mjModel.mesh_vert is float: widen it).  All NULL /
   * nmesh = 0: no meshes.  geom_dataid[g] = mesh of a MJPC_GEOM_MESH geom, -1 otherwise. */
  const int *geom_dataid, *mesh_vertadr, *mesh_vertnum;
  const double *mesh_vert;          /* [3 * nmeshvert] */
  /* height fields (geom_dataid[g] = height field of a MJPC_GEOM_HFIELD geom): nrow x ncol samples in [0, 1] (mjModel.hfield_data
   * is float: widen it), row-major with x along the columns; size = (radius_x, radius_y, elevation_z, base_z) */
  const int *hfield_nrow, *hfield_ncol, *hfield_adr;
  const double *hfield_size;        /* [4 * nhfield] */
  const double *hfield_data;        /* [nhfielddata] */
  /* keyframes */
  const double *key_qpos;           /* nkey * nq */
  const double *key_mpos;           /* nkey * 3*nmocap */
  /* added with ABI revision 4 */
  const int *actuator_refsite;      /* second mjModel.actuator_trnid int of a MJPC_TRN_SITE actuator: the reference site, -1 = none; NULL = none at
                                     * all.  With a reference site the transmission has a length (site position in the reference site's frame
                                     * dotted with gear[0:3]) and the moment (Jp_site - Jp_ref)^T R_ref gear[0:3], zero on the dofs both sites
                                     * share (mj_transmission); any gain / affine bias / activation state may ride it; a rotational gear
                                     * (gear[3:6] != 0) with a reference site is refused */
  double noslip_tolerance;          /* mjOption.noslip_tolerance (1e-6) */
} MjpcHipModel;

/* ---- task: cost table (mjpc/task.cc:147-245) + frozen ResidualFn state --------------- */
typedef struct MjpcHipTask {
  int struct_size;                  /* sizeof(MjpcHipTask) */
  int task_id;                      /* MJPC_TASK_* */
  int num_residual, num_term, num_trace;
  const int *dim_norm_residual;     /* [num_term] */
  const int *norm;                  /* [num_term] MJPC_NORM_* */
  const int *num_norm_parameter;    /* [num_term] */
  const double *weight;             /* [num_term] */
  const double *norm_parameter;     /* [sum num_norm_parameter] */
  double risk;
  int num_parameter;
  const double *parameters;         /* residual_* numerics, select values bit-cast (task.cc:38-64) */
  const int *trace_objtype;         /* [num_trace] MJPC_OBJ_SITE / BODY / GEOM (framepos sensors "trace%i") */
  const int *trace_objid;           /* [num_trace] */
  int num_int;  const int *int_data;      /* task-specific frozen ids  (layout: mjpc_hip_tasks.md / DESIGN.md) */
  int num_dbl;  const double *dbl_data;   /* task-specific frozen state */
} MjpcHipTask;

/* ---- one plan step ------------------------------------------------------------------- */
typedef struct MjpcHipPlanInput {
  /* State snapshot, mjpc/planners/sampling/planner.cc:146-149 */
  const double *state;      /* [nq+nv+na] */
  const double *mocap;      /* [7*nmocap] pos3+quat4 per mocap body */
  const double *userdata;   /* [nuserdata] */
  double time;
  /* nominal spline policy after UpdateNominalPolicy (planner.cc:236-310) */
  const double *knot_times;   /* [num_spline_points] */
  const double *knot_values;  /* [num_spline_points*nu] */
  int num_spline_points;
  int interpolation;          /* MJPC_SPLINE_* */
  /* sampling */
  int num_trajectory;         /* N: GLOBAL candidate count */
  int horizon;                /* H (steps, <= MJPC_MAX_HORIZON) */
  int candidate_offset;       /* first global candidate index owned by this engine (multi-GPU shard) */
  int num_local;              /* candidates rolled out by this engine: [offset, offset+num_local) */
  double noise_exploration[2];/* sigma; [1] used with prob. 0.2 when > 0 (planner.cc:320-325) */
  /* noise: explicit standard-normal tensor, or NULL -> Philox4x32-10(seed, stream) on device */
  const double *noise_eps;    /* [num_trajectory*P*nu] (global indexing) or NULL */
  const int *noise_sel;       /* [num_trajectory] 1 = use noise_exploration[1]; or NULL */
  uint64_t seed;
  uint64_t stream;            /* plan iteration counter */
  /* Cross-Entropy sampling (mjpc/planners/cross_entropy/planner.cc:340-375): when non-NULL, candidate knots are
   * nominal + noise_std[p*nu+k] * eps (absolute per-parameter std, no ctrlrange scaling), then clamped */
  const double *noise_std;    /* [num_spline_points*nu] or NULL (= SamplingPlanner noise above) */
  /* global index of the candidate that gets no noise: 0 for the SamplingPlanner (planner.cc:361); the Cross-Entropy
   * planner perturbs all N candidates and rolls the nominal out as candidate N of num_trajectory = N+1
   * (cross_entropy/planner.cc:377-415) */
  int nominal_index;
  /* Robust planner (mjpc/planners/robust/robust_planner.cc:91-157, Trajectory::NoisyRollout trajectory.cc:100-210):
   * explicit candidate policies and Ornstein-Uhlenbeck external-force noise on every body.
   * candidate_knots != NULL: candidate i uses candidate_knots[i] verbatim (no sampling noise at all).
   * xfrc_std > 0: before every step xfrc_applied = rate * xfrc_applied + N(0, xfrc_std * sqrt(1 - rate^2)),
   * rate = exp(-timestep / xfrc_rate) (trajectory.cc:147-155); normals from Philox(seed, stream ^ "XFRC", candidate i,
   * element t*6*nbody + k). */
  const double *candidate_knots;   /* [num_trajectory][num_spline_points][nu] (global indexing) or NULL */
  double xfrc_std, xfrc_rate;
} MjpcHipPlanInput;

typedef struct MjpcHipPlanOutput {
  /* all host buffers, caller-owned; any pointer may be NULL to skip the copy */
  double *returns;        /* [num_local] total_return per local candidate */
  int *failure;           /* [num_local] */
  int winner;             /* OUT: global index of local argmin (lowest index on ties) */
  double winner_return;   /* OUT */
  /* winner trajectory, same layout as mjpc::Trajectory (trajectory.h:74-86) */
  double *states;         /* [H*(nq+nv+na)] */
  double *actions;        /* [H*nu] */
  double *times;          /* [H] */
  double *residual;       /* [H*num_residual] */
  double *costs;          /* [H] */
  double *trace;          /* [H*3*num_trace] */
  double *winner_knots;   /* [P*nu] candidate_policy[winner].plan values */
  /* device timings of the last plan step, microseconds (fields mirror
   * noise_compute_time / rollouts_compute_time, planner.h:149-152) */
  double noise_compute_time_us;
  double rollouts_compute_time_us;
} MjpcHipPlanOutput;

typedef struct MjpcHipEngine MjpcHipEngine;

/* Create an engine on HIP device `device`.  Copies model+task to HBM.  max_local = largest
 * num_local that will be planned on this device.  Returns NULL on error (see last_error).
 * Models the engine cannot roll out faithfully are REFUSED here (never silently approximated): geom pairs without a
 * collider (height field against plane / height field; meshes / height fields without data), group-0 geoms the quadruped task's ground ray cannot hit, actuator transmissions other than joint /
 * fixed tendon, nconmax > 64, nefcmax > 192, iterations > 250, num_spline_points capacity 36, LDS footprint > 160 KiB. */
MjpcHipEngine *mjpc_hip_create(const MjpcHipModel *model, const MjpcHipTask *task,
                               int max_local, int max_horizon, int device);
void mjpc_hip_destroy(MjpcHipEngine *e);
/* Re-upload cost weights / norm params / residual parameters / frozen task state
 * (Agent::PlanIteration takes a fresh ResidualFn copy every plan step, agent.cc:290): only the task block travels,
 * as one stream-ordered asynchronous copy ahead of the next plan's kernels.  Error while a plan is in flight. */
int mjpc_hip_set_task(MjpcHipEngine *e, const MjpcHipTask *task);
/* One plan step: noise -> N rollouts -> costs -> argmin; blocking. 0 on success. */
int mjpc_hip_plan(MjpcHipEngine *e, const MjpcHipPlanInput *in, MjpcHipPlanOutput *out);
/* Split form used by bench.py / multi-GPU: enqueue on the engine's stream, then fetch.  One plan in flight per engine:
 * a second mjpc_hip_plan_async before mjpc_hip_plan_fetch is an error. */
int mjpc_hip_plan_async(MjpcHipEngine *e, const MjpcHipPlanInput *in);
int mjpc_hip_plan_fetch(MjpcHipEngine *e, MjpcHipPlanOutput *out);
/* What mjpc_hip_plan_fetch brings to the host.  MJPC_FETCH_WINNER_ROWS (default): returns, failure flags, and the local
 * winner's trajectory rows + knots in one packed copy.  MJPC_FETCH_SUMMARY: returns, failure flags, local winner index /
 * return / knots only — for the shards of a multi-device plan, where only the owner of the GLOBAL winner then copies its
 * trajectory with mjpc_hip_get_candidate. */
enum { MJPC_FETCH_WINNER_ROWS = 0, MJPC_FETCH_SUMMARY = 1 };
int mjpc_hip_set_fetch_mode(MjpcHipEngine *e, int mode);
/* Copy any local candidate's trajectory / knots to host (GUI traces, RankedPlanner). */
int mjpc_hip_get_candidate(MjpcHipEngine *e, int local_index, MjpcHipPlanOutput *out);
/* Copy every local candidate's knot values [num_local][P][nu] of the last plan to host (elite statistics of the
 * Cross-Entropy planner, cross_entropy/planner.cc:226-262). */
int mjpc_hip_get_knots(MjpcHipEngine *e, double *knots);
/* Every local candidate's trace rows [num_local][H][3*num_trace] of the last plan in one copy: what
 * SamplingPlanner::Traces draws (mjpc/planners/sampling/planner.cc:388-434). */
int mjpc_hip_get_traces(MjpcHipEngine *e, double *traces);
/* Every local candidate's Trajectory arrays of the last plan, [num_local][H][...] each (any pointer may be NULL): the
 * `trajectory[]` members other planners read (mjpc/planners/ilqs/planner.cc:98-198).  diag: [num_local][4] = Newton
 * iterations summed over the steps, max contacts, max constraint rows, MJPC_WARN_* bits. */
int mjpc_hip_get_all_candidates(MjpcHipEngine *e, double *states, double *actions, double *times, double *residual,
                                double *costs, double *trace, double *knots, int *diag);
/* ---- Sample-Gradient planner (mjpc/planners/sample_gradient/planner.cc) -------------------------------------------------
 * Its batch is mixed: one un-noised nominal (in->nominal_index), noisy candidates, then explicit policies; and its update needs
 * the standard normals themselves, which exist on the device only.  Three calls, one engine: there is no multi-device variant
 * (the planner drives one engine, like the Cross-Entropy planner).
 *
 * mjpc_hip_plan_mixed[_async]: a plan step whose candidates with global index < first_explicit are sampled as with
 * in->noise_std (required: nominal + noise_std * eps, clamped; bit for bit the rows a plain mjpc_hip_plan with noise_std gives)
 * and whose candidates >= first_explicit use in->candidate_knots[i] verbatim ([num_trajectory][P][nu], global indexing; rows
 * below first_explicit are not read; may be NULL when first_explicit == num_trajectory).  The table is assembled on the device
 * behind the noise kernel.  Fetch with mjpc_hip_plan_fetch; tiers, candidate_offset / num_local and mjpc_hip_get_* work as for
 * any plan.
 * Noise history: a device buffer [max_local][36 * nu], zero after create.  A mixed plan copies eps into slot r (local row) for
 * noisy rows only - nominal_index < global index < first_explicit - and only the first P * nu elements: slot 0, the explicit
 * slots and the tail of every slot keep what an earlier plan left (the reference's persistent `noise` vector, planner.cc:94,
 * 339-344).  mjpc_hip_noise_history_reset zeroes it (Planner::Reset, planner.cc:138).
 *
 * mjpc_hip_sample_gradient: gradient_out[k] = sum_{i<n} history[slot[i]][k] * scale[i] for k < P * nu, P of the last plan;
 * starts from 0.0, every product rounded and then added in ascending i (mju_addToScl, planner.cc:452-459): the result is the
 * reference loop's bit for bit, whatever the launch shape.  Blocking.  Errors: a plan in flight, no mixed plan yet, n outside
 * 1..max_local, a slot outside 0..max_local-1. */
int mjpc_hip_plan_mixed_async(MjpcHipEngine *e, const MjpcHipPlanInput *in, int first_explicit);
int mjpc_hip_plan_mixed(MjpcHipEngine *e, const MjpcHipPlanInput *in, int first_explicit, MjpcHipPlanOutput *out);
int mjpc_hip_noise_history_reset(MjpcHipEngine *e);
int mjpc_hip_sample_gradient(MjpcHipEngine *e, int n, const int *slot, const double *scale, double *gradient_out);
/* ---- Batched one-step evaluation and finite-difference transition derivatives ---------------------------------------------
 * What the reference's derivative-based planners spend their time in (mjpc/planners/model_derivatives.cc:45-165: one
 * mjd_transitionFD per knot, 1 + (2nv+na+nu) independent mj_steps one-sided, about twice that centred).  ds = nq+nv+na.
 *
 * mjpc_hip_step_batch: row i of `states` / `ctrl` / `time` is advanced by ONE step; next_states[i] is the state after it,
 * residual[i] the residual evaluated inside the step (at the pre-integration state with ctrl[i] applied, clamped to ctrlrange:
 * row 0 of a plan's residual), failure[i] the MJPC_WARN_* bits (0 = ok).  A row is bit for bit the first step of
 * mjpc_hip_plan(N = 1, H = 2, P = 1, candidate_knots = ctrl[i]) from states[i]: cold warm start, full-capacity kernel flavour.
 * mocap / userdata are shared by the batch.  n is unbounded: the batch runs in launches of at most max_local workgroups; an
 * engine created with max_horizon >= 2 serves it.  Blocking.  A failed row (bad state, full buffer) is not an error of the call:
 * its failure[i] is set, next_states[i] is the state it stopped at and residual[i] is NaN where the step never got there.
 * Errors (mjpc_hip_last_error): a plan in flight, n < 1, null inputs, max_horizon < 2.
 *
 * mjpc_hip_transition_fd: for each knot t < T, with nd = 2nv+na and nr = num_residual, row-major
 *   A[t][nd][nd] = d next / d state, B[t][nd][nu] = d next / d ctrl, C[t][nr][nd] = d residual / d state, D[t][nr][nu] = d residual / d ctrl,
 * entry [i][j] = d out_i / d in_j, tangent order [dq(nv), dv(nv), dact(na)] (mjd_transitionFD's).  A position nudge is the
 * engine's own position integration of a unit velocity over eps (hinge / slide / free translation: + eps; ball / free rotation:
 * right-multiplied by exp(eps e) and normalised); the position block of an output difference is the tangent between the two next
 * positions (quaternions: body-frame rotation vector of qa^-1 * qb), everything else a plain difference, each divided by eps or
 * 2 eps.  The residual differentiated is step_batch's.
 *   state columns    one-sided (y(+eps) - y(base)) / eps; centred (y(+eps) - y(-eps)) / (2 eps)
 *   control columns  with [lo, hi] the ctrlrange of a limited actuator: forward nudge iff not limited or u + eps <= hi; backward nudge
 *                    iff (centered || !forward) and (not limited or u - eps >= lo); both: centred formula; forward only:
 *                    (y+ - base) / eps; backward only: (base - y-) / eps; neither: a zero column
 * last_is_terminal: knot T-1 produces C only (state perturbations only); its A / B / D blocks are not written.
 * failure[t] = OR of the warning bits of every evaluation at t; the columns a failed evaluation feeds are left as computed.
 * T is unbounded (launches of at most max_local evaluations).  Blocking.  Errors: as above, and eps <= 0. */
int mjpc_hip_step_batch(MjpcHipEngine *e, int n, const double *states, const double *ctrl, const double *time, const double *mocap,
                        const double *userdata, double *next_states, double *residual, int *failure);
int mjpc_hip_transition_fd(MjpcHipEngine *e, int T, const double *x, const double *u, const double *time, const double *mocap,
                           const double *userdata, double eps, int centered, int last_is_terminal, double *A, double *B, double *C,
                           double *D, int *failure);
/* ---- Batched inverse dynamics and its finite-difference derivatives ----------------------------------------------------------
 * What the reference's direct trajectory optimiser and batch estimator spend their time in (mjpc/direct/direct.cc:1545-1576: one
 * mj_inverse per configuration of a window; :1717-1756: one mjd_inverseFD per configuration, 1 + 3nv independent inverse evaluations
 * one-sided, 1 + 6nv centred).  ds = nq+nv+na, nr = num_residual.
 *
 * mjpc_hip_inverse_batch: row i of `states` / `ctrl` / `qacc` / `time` is ONE inverse evaluation, no solver iteration in it:
 *   qfrc_constraint[i][nv] = J' f, f the force law of the step's constraint rows at jar = J a - aref (may be NULL)
 *   qfrc_inverse[i][nv]    = M a + qfrc_bias - qfrc_passive - qfrc_constraint: MuJoCo's meaning, actuator forces are NOT subtracted, so
 *                            the acceleration of a forward step gives back qfrc_actuator
 *   residual[i][nr]        the task residual at (qpos, qvel, act, ctrl) as mjpc_hip_step_batch reports it (may be NULL); the late rows
 *                            (accelerations, accelerometer / gyro / velocimeter, touch) are evaluated at the GIVEN acceleration and the
 *                            inverse constraint forces, as mj_sensorAcc does behind mj_inverse
 *   failure[i]             the MJPC_WARN_* bits (0 = ok): bad state, full contact / constraint buffers, and MJPC_WARN_BADQACC when
 *                            qacc[i] is not finite
 * discrete != 0 (mjENBL_INVDISCRETE, what direct/ sets): qacc is the discrete-time acceleration (v' - v) / timestep of a step and is first
 * converted to the continuous one, a = M^-1 (A qacc) with A the matrix the integrator solves with: M + timestep diag(damping) for Euler,
 * the same plus the tendon-damping / actuator-bias velocity terms for implicitfast (a term is skipped while its actuator's force sits on
 * its forcerange, as in the step), A = M without damping.  Then inverse_batch(discrete = 1) at (x, u, (v' - v) / timestep) of a forward
 * step returns that step's qfrc_actuator and qfrc_constraint up to the solver's convergence (models without a noslip pass).  Models with
 * the dense implicit integrators (MJPC_INT_IMPLICIT, implicitfast with fluid forces) are refused for discrete != 0: an error of the call,
 * no output is written.  mocap / userdata are shared by the batch.  n is unbounded (launches of at most max_local workgroups).
 * Blocking.  A failed row is not an error of the call: its failure[i] is set, and its outputs are NaN where the evaluation never got
 * there.  Errors: a plan in flight, n < 1, null inputs, max_horizon < 2, the refusal above.
 *
 * mjpc_hip_inverse_fd: for each configuration t < T, row-major, with f = qfrc_inverse and s = the residual of inverse_batch,
 *   DfDq[t][nv][nv], DfDv[t][nv][nv], DfDa[t][nv][nv], DsDq[t][nr][nv], DsDv[t][nr][nv], DsDa[t][nr][nv]      (any may be NULL)
 * entry [i][j] = d out_i / d in_j (mjd_inverseFD stores the transpose).  A position nudge is mjpc_hip_transition_fd's; velocities and
 * accelerations add eps; activations and controls are not differentiated.  One-sided (y(+eps) - y(base)) / eps, centred
 * (y(+eps) - y(-eps)) / (2 eps).  failure[t] = OR of the warning bits of every evaluation at t; the columns a failed evaluation feeds
 * are left as computed.  T is unbounded.  Blocking.  Errors: as above, and eps <= 0. */
int mjpc_hip_inverse_batch(MjpcHipEngine *e, int n, const double *states, const double *ctrl, const double *qacc, const double *time,
                           const double *mocap, const double *userdata, int discrete, double *qfrc_inverse, double *qfrc_constraint,
                           double *residual, int *failure);
int mjpc_hip_inverse_fd(MjpcHipEngine *e, int T, const double *states, const double *ctrl, const double *qacc, const double *time,
                        const double *mocap, const double *userdata, int discrete, double eps, int centered, double *DfDq, double *DfDv,
                        double *DfDa, double *DsDq, double *DsDv, double *DsDa, int *failure);
/* ---- State estimators: the device half of an unscented and an extended Kalman filter update ---------------------------------
 * mjpc/estimators/unscented.cc, kalman.cc.  nd = 2nv+na, ds = nq+nv+na.  The measurement is rows [sensor_first_row,
 * sensor_first_row + ns) of the engine's residual as mjpc_hip_step_batch reports it (the reference's estimator_sensor_start: one
 * task can carry cost rows and sensor rows).  Host pointers in and out, row-major.  Both calls are blocking.
 *
 * mjpc_hip_unscented_moments: the 2nd+1 sigma points around `state`, one step of each, and their weighted moments, in four stages
 * on the device with one upload and one download.  `factor` is a lower Cholesky factor L[nd][nd] of the covariance (entries above
 * the diagonal are not read); with c_i = sigma_step * L[:, i], row i < nd is state (+) c_i, row nd + i is state (-) c_i, row 2nd is
 * `state`, where (+) is the engine's position integration of the velocity c[0:nv] over time +-1 (a plain add on hinge, slide and
 * free-translation coordinates, on qvel and on act; quaternions are right-multiplied by exp(+-c) and normalised).  ctrl and time
 * are the same for every row.  weights = {mean0, cov0, sigma}: the nominal row's weight in the means, in the covariances, and
 * every other row's weight in both.
 *   state_mean[ds], sensor_mean[ns]   sum_j w_j y_j over the ascending row index j, one rounded product and one rounded add per step;
 *                     a quaternion's four numbers are instead the principal eigenvector of sum_j 4 w_j q_j q_j' - (sum_j w_j) I with the
 *                     covariance weights, its sign chosen so that its dot product with the nominal row's next quaternion is >= 0
 *   cov_ss[nd][nd], cov_sy[nd][ns], cov_yy[ns][ns]   noise_diag + sum_j (d_a[j] d_b[j]) w_j over ascending j, each operation rounded
 *                     separately, with d_j the difference of row j to the means (state part in tangent order: quaternion coordinates
 *                     the body-frame rotation vector of mean^-1 * q_j, everything else a plain difference); noise_process[nd] is the
 *                     diagonal added to ss, noise_sensor[ns] the one added to yy
 *   sigma_next[2nd+1][ds]   the next state of every row (may be NULL)
 *   *failure         OR of the rows' MJPC_WARN_* bits.  A failed row is not an error of the call.
 * Errors: a plan in flight, null inputs, max_horizon < 2, ns < 1, a row range outside num_residual.
 *
 * mjpc_hip_linearize_step: mjpc_hip_transition_fd at T = 1, last_is_terminal = 0, which also hands back the base evaluation it is
 * built around: next_state[ds] and residual[num_residual] are mjpc_hip_step_batch's of (state, ctrl, time), A[nd][nd] and
 * C[num_residual][nd] are transition_fd's.  Any output may be NULL.  One half-step of an extended Kalman filter is one call.
 * Errors: a plan in flight, null inputs, max_horizon < 2, eps <= 0. */
int mjpc_hip_unscented_moments(MjpcHipEngine *e, const double *state, const double *factor, double sigma_step, const double *weights,
                               const double *ctrl, double time, const double *mocap, const double *userdata, const double *noise_process,
                               const double *noise_sensor, int sensor_first_row, int ns, double *state_mean, double *sensor_mean,
                               double *cov_ss, double *cov_sy, double *cov_yy, double *sigma_next, int *failure);
int mjpc_hip_linearize_step(MjpcHipEngine *e, const double *state, const double *ctrl, double time, const double *mocap, const double *userdata,
                            double eps, int centered, double *next_state, double *residual, double *A, double *C, int *failure);
/* ---- Cost derivatives and the gradient planner's backward pass --------------------------------------------------------------
 * The other half of a derivative-based planner's iteration (mjpc/planners/cost_derivatives.cc, planners/gradient/gradient.cc),
 * on the device.  nd = 2nv+na, nr = num_residual; the cost table (norms, parameters, weights) and risk are the engine's current
 * task (mjpc_hip_set_task).  Host pointers in and out, row-major.
 *
 * mjpc_hip_cost_derivatives: for each knot t < T, with J = [C_t | D_t] and w_i = weight[i] / T, over the cost terms i in ascending
 * order and each term's own residual rows:  cr = the norm's gradient (Norm of mjpc/norm.cc, types -1, 0, 1, 2, 3, 5, 6, 7, 8),
 *   g = J_i' cr_i,  S = crr_i J_i,  G = J_i' S,  c{x,u} += w_i g,  c{xx,xu,uu} += w_i G   (Gauss-Newton)
 * cx[T][nd], cu[T][nu], cxx[T][nd][nd] the top-left block of G, cxu[T][nd][nu] the top-right, cuu[T][nu][nu] the bottom-right.
 * Summation: every contraction starts at 0.0 and runs over the ascending contraction index, one rounded product and one rounded
 * add per step (no fused multiply-add); `+= w_i v` is one rounded product and one rounded add; the Hessian of a type other than
 * 1 and 2 is diagonal and S its row scaling.  With |risk| >= 1e-6 and s = exp(risk * sum_i w_i Norm_i): cx and cu are scaled by s,
 * then c** = s c** + (risk s) (scaled c*) (scaled c*)' - the outer products use the ALREADY scaled gradients, as the reference does.
 * last_is_terminal: knot T-1 has no D (D[T-1] is not read): its cu, cuu, cxu are zero, cx and cxx come from C alone.
 * hessians = 0: cr, cx, cu only (cxx, cuu, cxu are not touched).  Any output may be NULL.  Blocking.
 * Errors: a plan in flight, T < 1, null inputs.
 *
 * mjpc_hip_trajectory_gradient: one iteration's derivative work with no host round trip in between: mjpc_hip_transition_fd over
 * the T knots with last_is_terminal = 1, the cost gradients (hessians = 0) over the matrices where that left them, with the
 * caller's residual[T][nr] (the nominal trajectory's), and Gradient::Compute:
 *   Vx[T-1] = cx[T-1];  for t = T-1 .. 1:  Qx[t-1] = A[t-1]' Vx[t] + cx[t-1],  Qu[t-1] = B[t-1]' Vx[t] + cu[t-1],
 *   k[t-1] = -Qu[t-1],  Vx[t-1] = Qx[t-1],  dV[0] += k[t-1] . Qu[t-1];   then k[T-1] = k[T-2];  dV[1] = 0
 * by the same summation rule, so a host loop over the downloaded matrices gives the same bits.  k[T][nu], Vx[T][nd], Qx[T-1][nd],
 * Qu[T-1][nu], dV[2] (any may be NULL), failure[T] as for mjpc_hip_transition_fd.  A failed evaluation is not an error of the call.
 * Blocking; one download.  Errors: a plan in flight, T < 2, null inputs, eps <= 0, max_horizon < 2, T beyond one pass of the step
 * tables (32768 evaluations). */
int mjpc_hip_cost_derivatives(MjpcHipEngine *e, int T, const double *residual, const double *C, const double *D, int last_is_terminal,
                              int hessians, double *cr, double *cx, double *cu, double *cxx, double *cuu, double *cxu);
int mjpc_hip_trajectory_gradient(MjpcHipEngine *e, int T, const double *x, const double *u, const double *time, const double *residual,
                                 const double *mocap, const double *userdata, double eps, int centered, double *k, double *Vx, double *Qx,
                                 double *Qu, double *dV, int *failure);
/* ---- The iLQG backward pass ---------------------------------------------------------------------------------------------------
 * mjpc/planners/ilqg/backward_pass.cc with its box-constrained control solve and the regularisation loop of ilqg/planner.cc:429-520,
 * in one kernel (csrc/riccati.h).  Host pointers, row-major: A [T-1][nd][nd], B [T-1][nd][nu] (or more blocks), cx [T][nd],
 * cxx [T][nd][nd] (index T-1 is the terminal knot), cu [T-1][nu], cxu [T-1][nd][nu], cuu [T-1][nu][nu] (or T blocks: the last is not
 * read), actions [T-1][nu] and action_limits [nu][2] (read when settings->action_limits == 1; an unlimited control has -inf, +inf).
 * A sweep runs t = T-2 .. 0 from Vx[T-1] = cx[T-1], Vxx[T-1] = cxx[T-1]; with W = Vxx[t+1], mu = *regularization:
 *   Qx = A'Vx[t+1] + cx,  Qu = B'Vx[t+1] + cu,  Qxx = (A'W)A + cxx,  Qxu = (A'W)B + cxu,  Quu = (B'W)B + cuu
 *   Quu_reg by regularization_type: 0 Quu + mu I; 1 Quu + mu B'B (both only when mu != 0); 2 (B'(W + mu I))B + cuu; other: Quu
 *   action_limits == 1: k = argmin 0.5 k'Quu_reg k + Qu'k over action_limits - actions[t] (projected Newton, warm-started from the
 *     previous knot's k, zero at the start of a call); K = -H_free^-1 Qxu_free' on the free controls, zero rows on the clamped ones
 *   else: K = -Quu_reg^-1 Qxu', k = -Quu_reg^-1 Qu by Cholesky; a pivot <= 0 fails the step   (Qxu is NOT regularised: the reference's)
 *   dV[0] += k.Qu,  dV[1] += 0.5 k'Quu k,  Vx[t] = Qx + K'(Quu k + Qu) + Qxu k,  Vxx[t] = sym(Qxx + K'QuuK + QxuK + K'Qxu')
 * A failed step ends the sweep: rate = max(rate * factor, factor), regularization = clamp(regularization * rate, min, max) (factor <= 1:
 * min in place of max for the rate), and the next sweep starts over with dV = 0, at most max_regularization_iterations times; a
 * regularisation above the maximum ends the call.  A complete sweep copies k[T-2], K[T-2] to index T-1.  status[3] = {1 complete / 0
 * failed, the failing time index (-1 when complete), regularisation increases}; a failed pass is not an error of the call: the outputs
 * hold what the sweeps stored (rows never reached are zero).  regularization / regularization_rate are in/out.
 * K [T][nu][nd], k [T][nu], Vx [T][nd], Vxx [T][nd][nd], Qx, Qu, Qxx, Qxu, Quu [T-1][..], dV [2]; any output may be NULL.  Summation
 * rule as for mjpc_hip_cost_derivatives, `/` and sqrt correctly rounded: mjpc_hip::iLQGBackwardPass on the host gives the same bits.
 * The engine lends its device and stream only (nd, nu are the caller's).  Blocking.  Errors: a plan in flight, T < 2, nd < 1, nu < 1,
 * null inputs, settings->struct_size.
 *
 * mjpc_hip_trajectory_ilqg: mjpc_hip_transition_fd (last_is_terminal = 1), the cost derivatives with Hessians where the matrices
 * lie, and the backward pass, with one download.  nd, nu and action_limits are the model's (an unlimited actuator gets -inf, +inf),
 * actions = the u rows.  Inputs and errors as for mjpc_hip_trajectory_gradient, plus a model without actuators. */
typedef struct MjpcHipRiccatiSettings {
  int struct_size;                        /* sizeof(MjpcHipRiccatiSettings) */
  int regularization_type;                /* 0 control, 1 state-control, 2 value, other: none */
  int action_limits;                      /* 1: box-QP over the action limits */
  int max_regularization_iterations;
  double min_regularization, max_regularization, regularization_factor;
} MjpcHipRiccatiSettings;
int mjpc_hip_ilqg_backward_pass(MjpcHipEngine *e, int T, int nd, int nu, const double *A, const double *B, const double *cx, const double *cu,
                                const double *cxx, const double *cxu, const double *cuu, const double *actions, const double *action_limits,
                                const MjpcHipRiccatiSettings *s, double *regularization, double *regularization_rate, double *k, double *K,
                                double *Vx, double *Vxx, double *Qx, double *Qu, double *Qxx, double *Qxu, double *Quu, double *dV, int *status);
int mjpc_hip_trajectory_ilqg(MjpcHipEngine *e, int T, const double *x, const double *u, const double *time, const double *residual,
                             const double *mocap, const double *userdata, double eps, int centered, const MjpcHipRiccatiSettings *s,
                             double *regularization, double *regularization_rate, double *k, double *K, double *Vx, double *Vxx, double *Qx,
                             double *Qu, double *Qxx, double *Qxu, double *Quu, double *dV, int *status, int *failure);
/* ---- The direct optimiser's window cost: gradient and band Hessian (mjpc/direct/direct.cc:683-1480, 1945-2106) -----------------------
 * A window is T >= 3 configurations of nv dofs; ntotal = nv T, nband = 3 nv.  Its cost is
 *   sum_t sum_i w_ti Norm_i(s_ti - y_ti)  +  sum_{0 < t < T-1} 0.5 (f_t - tau_t)' diag(w_f) (f_t - tau_t)
 * over the sensors i (runs of rows of the engine's residual, starting at sensor_first_row, as for mjpc_hip_unscented_moments) and the
 * inverse-dynamics force f, with v_t = differentiatePos(q_{t-1}, q_t) / h and a_t = (v_{t+1} - v_t) / h, so that configuration t's
 * terms depend on q_{t-1}, q_t, q_{t+1} alone and the Gauss-Newton Hessian is banded.
 *   w_ti = time_weight / noise_sensor[i] / sensor_dim[i] / T, time_weight = 1 / h^2 / h^4 for a position / velocity / acceleration stage
 *     sensor under time_scaling_sensor (else 1); times first_step_position_sensors at t = 0, times (last_step_position_sensors ||
 *     last_step_velocity_sensors) at t = T - 1; a sensor whose sensor_mask[t][i] is 0 is left out
 *   w_f[j] = h^4 / noise_process[j] / nv / (T - 2) (1 in place of h^4 without time_scaling_force)
 *   at t = 0 the residual of every sensor that is not position stage is zero; at t = T - 1 a position (velocity) stage sensor's
 *     residual stays under last_step_position_sensors (last_step_velocity_sensors), every other is zero
 * sensor_stage: 0 position, 1 velocity, 2 acceleration.  sensor_norm / sensor_norm_parameter [num_sensor][2]: the cost table's norm
 * types and {p, q}.
 *
 * mjpc_hip_direct_assemble: the algebra alone, on the caller's arrays.
 *   in   residual_sensor [T][ns] = prediction - measurement, residual_force [T][nv] (rows 0 and T - 1 are not read), before any
 *        zeroing; the six blocks of mjpc_hip_inverse_fd, [T][nv][nv] and [T][nr][nv], as that call returns them: the ends' rules of
 *        mjpc_hip::InverseDerivatives (t = 0 keeps the position-stage rows of DsDq alone; t = T - 1 keeps DsDq and DsDv without their
 *        acceleration-stage rows) are applied here, to what is read; dvdq0, dvdq1 [T][nv][nv] = dv_t/dq_{t-1}, dv_t/dq_t (index 0 is
 *        not read)
 *   out  cost [3] = {cost, cost_sensor, cost_force}; gradient [ntotal]; hessian_band [ntotal][nband], MuJoCo's lower band (row R
 *        holds columns R - nband + 1 .. R, the diagonal at column nband - 1, leading zeros in front of column 0)
 *   optional (NULL: not copied)  block_sensor [T][ns][nband], block_force [T][nv][nband]: configuration t's Jacobian, column c standing
 *        for global column nv (t - 1) + c (t = 0: columns nv .. 2 nv alone; t = T - 1: the first 2 nv; what a configuration does
 *        not have is zero); norm_gradient_sensor [T][ns], norm_gradient_force [T][nv] (the latter weighted, as the reference's);
 *        residual_sensor_out [T][ns], residual_force_out [T][nv]: the residuals behind the zeroing rules
 * One owner per output entry; an entry's sensor part is summed over ascending t and within t over ascending sensor, its force part
 * over ascending t, the total is sensor + force, by the summation rule of mjpc_hip_cost_derivatives (`/` and sqrt correctly rounded):
 * no atomics, two calls give the same bits, mjpc_hip::DirectCost::AssembleHost gives the same bits.  The engine lends its device and
 * stream only (nv, nr are the caller's).  Blocking.  Errors, before anything is touched: a plan in flight, T < 3, nv < 1, null inputs,
 * settings->struct_size, num_sensor < 0, a sensor dimension < 1, dimensions that do not sum to num_sensor_rows, sensor rows outside
 * [0, nr), a stage outside 0 .. 2, a noise value <= 0, timestep <= 0. */
typedef struct MjpcHipDirectSettings {
  int struct_size;                        /* sizeof(MjpcHipDirectSettings) */
  int num_sensor, sensor_first_row, num_sensor_rows;
  const int *sensor_dim, *sensor_stage, *sensor_norm;     /* [num_sensor] */
  const double *sensor_norm_parameter;    /* [num_sensor][2] */
  const double *noise_sensor;             /* [num_sensor] */
  const double *noise_process;            /* [nv] */
  const int *sensor_mask;                 /* [T][num_sensor]; NULL: every sensor on */
  int sensor_flag, force_flag, time_scaling_sensor, time_scaling_force;
  int first_step_position_sensors, last_step_position_sensors, last_step_velocity_sensors;
  double timestep;                        /* h */
} MjpcHipDirectSettings;
/* mjpc_hip_direct_cost: the cost alone of nwin >= 1 candidate windows in one call (a line search is one launch of the inverse kernel over
 * nwin T rows): q [nwin][T][nq], act [nwin][T][na], ctrl [nwin][T][nu] per window; time [T], sensor_measurement [T][ns],
 * force_measurement [T][nv], the mask, mocap and userdata are shared.  On the device: the windows' rows (v_t = differentiatePos(q_{t-1},
 * q_t) / h, a_t = (v_{t+1} - v_t) / h, a quaternion dof's velocity the body-frame rotation vector in the feedback rollouts' spelling; v_0
 * = a_0 = a_{T-1} = 0) written into the inverse kernel's table, the existing inverse kernel, the residuals, norms and one reduction per
 * window.  cost [nwin][3] = {cost, cost_sensor, cost_force}; optional (NULL: not copied) velocity, acceleration [nwin][T][nv],
 * sensor_prediction [nwin][T][ns], force_prediction [nwin][T][nv], failure [nwin][T] (the evaluation's MJPC_WARN_* bits: they do not stop
 * the call).  settings->timestep is h.
 *
 * mjpc_hip_direct_cost_derivatives: one window, everything on the device with nothing downloaded in between: the window's rows and the
 * velocity blocks dv_t/dq_{t-1}, dv_t/dq_t (-1/h, 1/h on plain coordinates, the 3 x 3 blocks of the quaternion difference over h on ball
 * and free-rotation dofs, with the reference's swapped argument order), mjpc_hip_inverse_fd's table, evaluations and differences, the
 * residuals of the base evaluations, and the algebra of mjpc_hip_direct_assemble on the blocks where they lie.  Required: cost [3],
 * gradient, hessian_band; every other output is optional.  failure [T].  The costs are the bits mjpc_hip_direct_cost gives for the
 * same window.
 * Errors of both, before anything is touched: those of mjpc_hip_direct_assemble, nwin < 1, fd_eps <= 0, discrete != 0 on an int_dense
 * model (as mjpc_hip_inverse_fd), a window beyond one pass of the inverse tables, a plan in flight. */
int mjpc_hip_direct_cost(MjpcHipEngine *e, int nwin, int T, const MjpcHipDirectSettings *s, int discrete, const double *q, const double *act,
                         const double *ctrl, const double *time, const double *sensor_measurement, const double *force_measurement,
                         const double *mocap, const double *userdata, double *cost, double *velocity, double *acceleration,
                         double *sensor_prediction, double *force_prediction, int *failure);
int mjpc_hip_direct_cost_derivatives(MjpcHipEngine *e, int T, const MjpcHipDirectSettings *s, double fd_eps, int centered, int discrete,
                                     const double *q, const double *act, const double *ctrl, const double *time, const double *sensor_measurement,
                                     const double *force_measurement, const double *mocap, const double *userdata, double *cost, double *gradient,
                                     double *hessian_band, double *block_sensor, double *block_force, double *norm_gradient_sensor,
                                     double *norm_gradient_force, double *residual_sensor, double *residual_force, double *DfDq, double *DfDv,
                                     double *DfDa, double *DsDq, double *DsDv, double *DsDa, double *dvdq0, double *dvdq1, int *failure);
int mjpc_hip_direct_assemble(MjpcHipEngine *e, int T, int nv, int nr, const MjpcHipDirectSettings *s, const double *residual_sensor,
                             const double *residual_force, const double *DfDq, const double *DfDv, const double *DfDa, const double *DsDq,
                             const double *DsDv, const double *DsDa, const double *dvdq0, const double *dvdq1, double *cost, double *gradient,
                             double *hessian_band, double *block_sensor, double *block_force, double *norm_gradient_sensor,
                             double *norm_gradient_force, double *residual_sensor_out, double *residual_force_out);
/* ---- Rollouts under a feedback policy (iLQG's ActionRollouts / FeedbackRollouts, mjpc/planners/ilqg/planner.cc:618-712) ------------
 * Candidate i of the batch applies at step t < H-1, with x_t its own state at that step,
 *   u = clamp( (ubar[t] + action_step[i] * kbar[t]) + feedback_scaling[i] * ( Kbar[t] * StateDiff(xbar[t], x_t) ), ctrlrange )
 * StateDiff = mj_differentiatePos over the positions (quaternions: body-frame rotation vector of xbar^-1 x) and plain differences
 * of velocities and activations, tangent order [dq(nv), dv(nv), dact(na)]; nd = 2nv+na, ds = nq+nv+na.
 *   mode MJPC_FEEDBACK_INDEXED: ubar[t], kbar[t], xbar[t], Kbar[t] are row t of the policy's arrays (T >= H)  - Trajectory::RolloutDiscrete
 *   mode MJPC_FEEDBACK_TIME:    they are the policy interpolated at the step's time (zero / linear / cubic by `representation`, the
 *     actions, improvement and gains over the first T-1 knots, the states over all T with their quaternions renormalised; zero-order
 *     outside the knots): iLQGPolicy::Action.  The step times are in->time + t timesteps, accumulated as the rollout does; the
 *     tables are resampled once per call on the device, the rollout never interpolates.
 * use_feedback = 0 skips the feedback term (it is not multiplied by zero); action_improvement = NULL skips the action_step term.
 * Arithmetic: mjpc_hip::iLQGPolicy::Action's - every row of Kbar dx from 0.0 in ascending index with one rounded product and one rounded
 * add, each scaled add one product and one add, the clamp last - so the recorded action of a step equals that function at the recorded
 * state of the step bit for bit (the angle of a quaternion tangent comes from one correctly rounded atan2 that host and device share,
 * csrc/atan2_cr.h, not from either side's math library).
 * Of `in` only state, mocap, userdata, time, horizon, num_trajectory and candidate_offset are read: the engine rolls out the candidates
 * [candidate_offset, num_trajectory).  Full capacity only
 * (no dense tier): the reference caps the batch at kMaxTrajectory = 128.  Outputs, mjpc_hip_plan_fetch and the mjpc_hip_get_* calls
 * behave as after mjpc_hip_plan; there are no knots (winner_knots is left untouched, mjpc_hip_get_knots copies nothing).
 * Errors: a plan in flight, a batch above the engine's max_local (max_samples), horizon out of range, T < 2, indexed mode with T < H, an unknown mode or
 * representation, null arrays, a NaN in action_step / feedback_scaling, policy->struct_size. */
enum { MJPC_FEEDBACK_INDEXED = 0, MJPC_FEEDBACK_TIME = 1 };
typedef struct MjpcHipFeedbackPolicy {
  int struct_size;                  /* sizeof(MjpcHipFeedbackPolicy) */
  int mode;                         /* MJPC_FEEDBACK_* */
  int T;                            /* number of knots */
  int representation;               /* MJPC_SPLINE_* (0 zero, 1 linear, 2 cubic): read in MJPC_FEEDBACK_TIME mode */
  const double *times;              /* [T] */
  const double *states;             /* [T][ds] */
  const double *actions;            /* [T][nu] */
  const double *feedback_gain;      /* [T][nu][nd] */
  const double *action_improvement; /* [T][nu] or NULL */
  const double *action_step;        /* [num_trajectory] alpha_i (global indexing) */
  const double *feedback_scaling;   /* [num_trajectory] s_i (global indexing) */
  int use_feedback;                 /* 0: no feedback term (the reference's state == NULL) */
} MjpcHipFeedbackPolicy;
int mjpc_hip_plan_feedback_async(MjpcHipEngine *e, const MjpcHipPlanInput *in, const MjpcHipFeedbackPolicy *policy);
int mjpc_hip_plan_feedback(MjpcHipEngine *e, const MjpcHipPlanInput *in, const MjpcHipFeedbackPolicy *policy, MjpcHipPlanOutput *out);
/* Device time of the last call's resampling kernel in microseconds (0 in indexed mode); valid after the fetch. */
double mjpc_hip_feedback_resample_time_us(MjpcHipEngine *e);
int mjpc_hip_sizeof_feedback_policy(void);
/* Bytes of the backward-pass kernel's work image at (nd, nu), and where it lies: *in_lds = 1 in the workgroup's LDS (up to 160 KiB),
 * 0 in a global-memory scratch of the same layout.  Host only, no GPU needed. */
int mjpc_hip_riccati_layout_bytes(int nd, int nu, int *in_lds);
/* Bytes of LDS one candidate's workgroup occupies (its whole mjData-equivalent). */
int mjpc_hip_lds_bytes(MjpcHipEngine *e);
/* Capacity tiers: when a shard holds more candidates than the GPU has CUs and the model allows it, the engine first runs a
 * flavour that fits TWO candidates per CU (<= 80 KiB of LDS each, smaller contact / row capacity) and re-runs the rare
 * candidate that overflowed it at full capacity - same results, ~1.6x the throughput.  Returns the dense tier's LDS bytes
 * (0: none for this model); *used_last = 1 when the last plan used it. */
int mjpc_hip_dense_tier(MjpcHipEngine *e, int *used_last);
/* The same figure for a model without creating an engine (host-only, no GPU needed): with (1) / without (0) the LDS copy of
 * the model tables; use_cache | 2: the dense tier's lean layout at the model's nefcmax / nconmax.  Negative: mjpc_hip_create
 * would refuse the model or the views (struct_size) (see mjpc_hip_last_error). */
int mjpc_hip_layout_bytes(const MjpcHipModel *model, const MjpcHipTask *task, int use_cache);
/* Kinematic frame of local candidate 0 at the first step of the last plan (the state handed in): what a host-side
 * Task::Transition reads from mjData after a simulation step (mjpc/tasks/quadruped/quadruped.cc:254,290-330: body poses, site
 * positions, subtree com / linear velocity sensors).  Any pointer may be NULL.  Sizes: xpos 3*nbody, xmat 9*nbody,
 * site_xpos 3*nsite, subtree_com 3*nbody, subtree_linvel 3*nbody. */
int mjpc_hip_get_frame(MjpcHipEngine *e, double *xpos, double *xmat, double *site_xpos, double *subtree_com, double *subtree_linvel);
/* Average device time of the rollout kernel over the launches since the last call,
 * measured with hipEvents on the engine's stream; returns launches counted. */
int mjpc_hip_kernel_time(MjpcHipEngine *e, double *avg_rollout_us, double *avg_total_us);
/* Device pointers of the last plan's result arrays (for zero-copy consumers / tests). */
int mjpc_hip_device_ptrs(MjpcHipEngine *e, void **returns, void **states, void **residual);
/* ---- one planner, several GPUs (north_star: "candidate batches shard across the 8 GPUs of one node") -------------------
 * A MjpcHipMulti owns one engine per device in ONE host process (the planner lives in one process, planners/include.cc:44).
 * mjpc_hip_multi_plan block-partitions the global batch [0, num_trajectory) over the engines (candidate 0, the un-noised
 * nominal, on the first), enqueues every shard asynchronously on its device's stream, fetches the per-shard summaries
 * (returns + local elite, MJPC_FETCH_SUMMARY), takes the lexicographic minimum (return, global index) on the host - G x 16
 * bytes that are on the host anyway with returns[]; an RCCL collective would add a launch + sync per device for nothing -
 * and copies the winner's trajectory from its owner only.  Results are bit-identical to one engine planning the whole batch
 * (noise is indexed by the global candidate id).  `devices`: n_devices HIP device ordinals (repeats allowed: several
 * engines on one GPU, used by the 1-GPU rehearsal test); NULL = 0 .. n_devices-1.  in->candidate_offset / num_local are
 * ignored (the whole batch is planned); out->returns / failure are [num_trajectory]. */
typedef struct MjpcHipMulti MjpcHipMulti;
MjpcHipMulti *mjpc_hip_multi_create(const MjpcHipModel *model, const MjpcHipTask *task, int max_samples, int max_horizon,
                                    int n_devices, const int *devices);
void mjpc_hip_multi_destroy(MjpcHipMulti *m);
int mjpc_hip_multi_set_task(MjpcHipMulti *m, const MjpcHipTask *task);
int mjpc_hip_multi_plan(MjpcHipMulti *m, const MjpcHipPlanInput *in, MjpcHipPlanOutput *out);
/* trajectory / knots of GLOBAL candidate `index` of the last plan, from the engine that owns it */
int mjpc_hip_multi_get_candidate(MjpcHipMulti *m, int index, MjpcHipPlanOutput *out);
/* knots [num_trajectory][P][nu] / traces [num_trajectory][H][3*num_trace] of every candidate of the last plan */
int mjpc_hip_multi_get_knots(MjpcHipMulti *m, double *knots);
int mjpc_hip_multi_get_traces(MjpcHipMulti *m, double *traces);
int mjpc_hip_multi_num_devices(const MjpcHipMulti *m);
/* engine k (0 .. n_devices-1), e.g. for mjpc_hip_get_frame / mjpc_hip_kernel_time */
MjpcHipEngine *mjpc_hip_multi_engine(MjpcHipMulti *m, int k);
const char *mjpc_hip_last_error(void);
int mjpc_hip_version(void);                 /* MJPC_HIP_ABI_VERSION of the library */
int mjpc_hip_sizeof_model(void);
int mjpc_hip_sizeof_task(void);
int mjpc_hip_sizeof_plan_input(void);
int mjpc_hip_sizeof_plan_output(void);

#ifdef __cplusplus
}
#endif
#endif  /* MJPC_HIP_H_ */
