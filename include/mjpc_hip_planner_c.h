/* mjpc_hip_planner_c.h — flat C view of the C++ host planner (include/mjpc_hip_planner.h), exported by
 * libmjpc_hip.so for bindings that cannot take C++ classes (ctypes tests, the Python front end).
 * Each function forwards to the method of the same name; the reference interface each one stands for:
 *   mjpc_spline_*   -> mjpc::spline::TimeSpline              (mjpc/spline/spline.h:41-276)
 *   mjpc_planner_*  -> mjpc::SamplingPlanner / RankedPlanner (mjpc/planners/sampling/planner.h:51-162,
 *                                                             mjpc/planners/planner.h:38-101)
 *   mjpc_cem_* / mjpc_robust_* / mjpc_sg_* -> CrossEntropyPlanner / RobustPlanner / SampleGradientPlanner
 *   mjpc_md_*       -> mjpc::ModelDerivatives                 (mjpc/planners/model_derivatives.h:30-70)
 *   mjpc_id_*       -> mjpc::Direct::InverseDynamicsDerivatives (mjpc/direct/direct.cc:1641-1830)
 *   mjpc_dc_*       -> mjpc::Direct::Cost with gradient and band Hessian, the algebra on given blocks (mjpc/direct/direct.cc:683-1480, 1945-2106)
 *   mjpc_cd_* / mjpc_gd_* -> mjpc::CostDerivatives, mjpc::Gradient (mjpc/planners/cost_derivatives.h, planners/gradient/gradient.h)
 *   mjpc_ilqg_* / mjpc_ilqs_* -> mjpc::iLQGPlanner, mjpc::iLQSPlanner (mjpc/planners/ilqg/planner.h, planners/ilqs/planner.h)
 * Handles are opaque; errors go through the installed handler (default: print + abort, like mju_error).
 */
#ifndef MJPC_HIP_PLANNER_C_H_
#define MJPC_HIP_PLANNER_C_H_
#include "mjpc_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

void mjpc_planner_set_error_handler(void (*handler)(const char *message));

/* TimeSpline */
void *mjpc_spline_create(int dim, int interpolation);
void mjpc_spline_destroy(void *spline);
int mjpc_spline_size(void *spline);
void mjpc_spline_add_node(void *spline, double time, const double *values /* NULL = zeros */);
void mjpc_spline_sample(void *spline, double time, double *out /* [dim] */);
int mjpc_spline_discard_before(void *spline, double time);
void mjpc_spline_clear(void *spline);
void mjpc_spline_set_interpolation(void *spline, int interpolation);

/* SamplingPlanner: create = Initialize + Allocate (planner.cc:40-133) */
void *mjpc_planner_create(const MjpcHipModel *model, const MjpcHipTask *task, const double *exploration /* [2] */,
                          int trajectories, int representation, int sliding_plan, int spline_points,
                          int max_samples, int max_horizon, int device);
/* the same planner with the candidate batch of every plan step sharded over n_devices GPUs (one engine each, elite picked
 * across them; devices[k] = HIP ordinals, repeats allowed for a 1-GPU rehearsal) */
void *mjpc_planner_create_sharded(const MjpcHipModel *model, const MjpcHipTask *task, const double *exploration /* [2] */,
                                  int trajectories, int representation, int sliding_plan, int spline_points,
                                  int max_samples, int max_horizon, int n_devices, const int *devices);
void mjpc_planner_destroy(void *planner);
void mjpc_planner_reset(void *planner, int horizon, const double *initial_repeated_action);
void mjpc_planner_set_state(void *planner, const double *state, const double *mocap, const double *userdata, double time);
void mjpc_planner_set_task(void *planner, const MjpcHipTask *task);
void mjpc_planner_optimize_policy(void *planner, int horizon);
void mjpc_planner_nominal_trajectory(void *planner, int horizon);
void mjpc_planner_action_from_policy(void *planner, double *action, double time, int use_previous);
int mjpc_planner_optimize_policy_candidates(void *planner, int ncandidates, int horizon);
double mjpc_planner_candidate_score(void *planner, int candidate);
void mjpc_planner_action_from_candidate_policy(void *planner, double *action, int candidate, double time);
void mjpc_planner_copy_candidate_to_policy(void *planner, int candidate);
int mjpc_planner_winner(void *planner);
double mjpc_planner_improvement(void *planner);
int mjpc_planner_num_parameters(void *planner);
void mjpc_planner_set_seed(void *planner, unsigned long long seed, unsigned long long plan_iter);
void mjpc_planner_set_num_trajectory(void *planner, int num_trajectory);
void mjpc_planner_set_noise(void *planner, const double *eps, const int *sel);   /* borrowed until the next call */
void mjpc_planner_returns(void *planner, double *out, int n);
int mjpc_planner_policy(void *planner, int previous, double *times, double *values);          /* returns P */
int mjpc_planner_best_trajectory(void *planner, double *states, double *actions, double *times, double *residual,
                                 double *costs, double *trace, double *total_return, int *failure); /* returns H */
void mjpc_planner_timings(void *planner, double *noise_us, double *rollouts_us, double *policy_update_us);

/* CrossEntropyPlanner (mjpc/planners/cross_entropy/planner.h:32-147): create = Initialize + Allocate */
void *mjpc_cem_create(const MjpcHipModel *model, const MjpcHipTask *task, double std_initial, double std_min, int trajectories,
                      int n_elite, int representation, int spline_points, int max_samples, int max_horizon, int device);
void mjpc_cem_destroy(void *planner);
void mjpc_cem_reset(void *planner, int horizon, const double *initial_repeated_action);
void mjpc_cem_set_state(void *planner, const double *state, const double *mocap, const double *userdata, double time);
void mjpc_cem_set_seed(void *planner, unsigned long long seed, unsigned long long plan_iter);
void mjpc_cem_set_noise(void *planner, const double *eps);     /* borrowed until the next call */
void mjpc_cem_optimize_policy(void *planner, int horizon);
void mjpc_cem_nominal_trajectory(void *planner, int horizon);
void mjpc_cem_action_from_policy(void *planner, double *action, double time, int use_previous);
double mjpc_cem_improvement(void *planner);
void mjpc_cem_returns(void *planner, double *out, int n);
void mjpc_cem_variance(void *planner, double *out, int n);
int mjpc_cem_policy(void *planner, double *times, double *values);                               /* returns P */
int mjpc_cem_best_trajectory(void *planner, double *states, double *actions, double *costs, double *total_return);   /* returns H */

/* RobustPlanner (mjpc/planners/robust/robust_planner.h:31-80) over a SamplingPlanner delegate */
void *mjpc_robust_create(const MjpcHipModel *model, const MjpcHipTask *task, const double *exploration, int trajectories, int representation,
                         int spline_points, int repetitions, int candidates, double xfrc_std, double xfrc_rate, int max_samples,
                         int max_horizon, int device);
void mjpc_robust_destroy(void *planner);
void mjpc_robust_reset(void *planner, int horizon);
void mjpc_robust_set_state(void *planner, const double *state, const double *mocap, const double *userdata, double time);
void mjpc_robust_set_seed(void *planner, unsigned long long delegate_seed, unsigned long long robust_seed, unsigned long long plan_iter);
void mjpc_robust_optimize_policy(void *planner, int horizon);
void mjpc_robust_action_from_policy(void *planner, double *action, double time);
void mjpc_robust_last(void *planner, int *out /* [3] best, ncand, rep */, double *scores, double *noisy_returns);
void *mjpc_robust_delegate(void *planner);     /* the SamplingPlanner handle (mjpc_planner_* calls), owned by the robust planner */

/* SampleGradientPlanner (mjpc/planners/sample_gradient/planner.h:35-175): create = Initialize + Allocate */
void *mjpc_sg_create(const MjpcHipModel *model, const MjpcHipTask *task, double exploration, int trajectories, int gradient_trajectories,
                     double gradient_filter, int representation, int spline_points, int max_samples, int max_horizon, int device);
void mjpc_sg_destroy(void *planner);
void mjpc_sg_reset(void *planner, int horizon, const double *initial_repeated_action);
void mjpc_sg_set_state(void *planner, const double *state, const double *mocap, const double *userdata, double time);
void mjpc_sg_set_task(void *planner, const MjpcHipTask *task);
void mjpc_sg_set_seed(void *planner, unsigned long long seed, unsigned long long plan_iter);
void mjpc_sg_set_noise(void *planner, const double *eps);      /* [num_trajectory * P * nu] standard normals, borrowed until the next call */
void mjpc_sg_set_counts(void *planner, int trajectories, int gradient_trajectories);   /* the GUI sliders num_trajectory_ / num_gradient_ */
void mjpc_sg_optimize_policy(void *planner, int horizon);
void mjpc_sg_nominal_trajectory(void *planner, int horizon);
void mjpc_sg_action_from_policy(void *planner, double *action, double time, int use_previous);
double mjpc_sg_improvement(void *planner);
int mjpc_sg_winner(void *planner);
int mjpc_sg_winner_type(void *planner);                        /* 0 nominal, 1 perturbed, 2 gradient */
int mjpc_sg_num_gradient(void *planner);                       /* num_gradient_ after its clamp */
int mjpc_sg_num_parameters(void *planner);
void mjpc_sg_returns(void *planner, double *out, int n);
void mjpc_sg_trajectory_order(void *planner, int *out, int n);
void mjpc_sg_gradient(void *planner, double *out, int n);
int mjpc_sg_return_weight(void *planner, double *out /* NULL: size only */);   /* return_weight_; returns its size */
int mjpc_sg_step_size(void *planner, double *out /* NULL: size only */);       /* step_size_; returns its size */
int mjpc_sg_policy(void *planner, double *times, double *values);                                  /* returns P */
int mjpc_sg_candidate_policy(void *planner, int index, double *times, double *values);             /* candidate_policy[index]; returns P */
int mjpc_sg_best_trajectory(void *planner, double *states, double *actions, double *costs, double *total_return);   /* returns H */
void mjpc_sg_timings(void *planner, double *noise_us, double *rollouts_us, double *policy_update_us, double *gradient_candidates_us);
/* the planner's host closed forms without a planner (no GPU needed): fitness-shaping weights over an order of candidate indices
 * (planner.cc:437-449) and LogScale (utilities.cc:802-808) */
void mjpc_sg_return_weights(const int *order, int num_noisy, double *weights);
void mjpc_sg_log_scale(double *values, double max_value, double min_value, int steps);

/* ModelDerivatives (mjpc/planners/model_derivatives.h:30-70): create = Allocate + Reset.  The engine is the caller's (mjpc_hip_create,
 * max_horizon >= 2). */
void *mjpc_md_create(int dim_state /* nq + nv + na */, int dim_state_derivative, int dim_action, int dim_sensor, int T);
void mjpc_md_destroy(void *md);
void mjpc_md_reset(void *md, int T);
/* 0 = ok, -1 = refused (T < 2: through the error handler) or engine error (mjpc_hip_last_error) */
int mjpc_md_compute(void *md, MjpcHipEngine *engine, const double *x, const double *u, const double *h, int T, double tol, int mode, int skip,
                    const double *mocap, const double *userdata);
/* the host halves without an engine (no GPU needed): the index sets of (T, skip); every interpolated block from the evaluated ones */
void mjpc_md_index_sets(void *md, int T, int skip);
void mjpc_md_interpolate(void *md);
/* evaluate_ into evaluate[] and interpolate_ into interpolate[] (either may be NULL); returns their sizes in n[2] */
void mjpc_md_indices(void *md, int *evaluate, int *interpolate, int *n);
/* the first T blocks: store != 0 copies the arrays INTO the object (tests fill the evaluated blocks), else out of it; any pointer may be NULL */
void mjpc_md_blocks(void *md, int T, int store, double *A, double *B, double *C, double *D, int *failure);

/* InverseDerivatives (mjpc/direct/direct.cc:1641-1830, Direct::InverseDynamicsDerivatives): the six blocks of mjpc_hip_inverse_fd along a
 * window, with the window's ends as the reference keeps them (include/mjpc_hip_planner.h).  create = Allocate + Reset. */
void *mjpc_id_create(int dim_state /* nq + nv + na */, int nq, int nv, int dim_action, int dim_sensor, int T);
void mjpc_id_destroy(void *id);
/* stage[dim_sensor] of 0 (position), 1 (velocity), 2 (acceleration); from a MJPC_TASK_TABLE task: 0 = ok, -1 = not a table of dim_sensor rows */
void mjpc_id_set_row_stages(void *id, const int *stage);
int mjpc_id_row_stages_from_table(void *id, const MjpcHipTask *task);
void mjpc_id_row_stages(void *id, int *stage);
/* 0 = ok, -1 = refused (T < 1: through the error handler) or engine error (mjpc_hip_last_error) */
int mjpc_id_compute(void *id, MjpcHipEngine *engine, const double *x, const double *u, const double *a, const double *h, int T, double tol, int mode,
                    int discrete, const double *mocap, const double *userdata);
/* the first T blocks out of the object; any pointer may be NULL */
void mjpc_id_blocks(void *id, int T, double *DfDq, double *DfDv, double *DfDa, double *DsDq, double *DsDv, double *DsDa, int *failure);

/* DirectCost (mjpc/direct/direct.cc:683-1480, 1945-2106, Direct::Cost with gradient and Hessian): the window's cost, gradient and band
 * Hessian from the residuals, the six blocks of mjpc_id_* and the velocity blocks.  set_settings: flags [7] = sensor_flag, force_flag,
 * time_scaling_sensor, time_scaling_force, first_step_position_sensors, last_step_position_sensors, last_step_velocity_sensors.
 * assemble: on the device through mjpc_hip_direct_assemble, or with engine == NULL on the host (DirectCost::AssembleHost, the same
 * bits); 0 = ok, -1 = refused (mjpc_hip_last_error / the planner's error handler).  outputs: any pointer may be NULL. */
void *mjpc_dc_create(int nv, int nr, int T);
void mjpc_dc_destroy(void *dc);
void mjpc_dc_set_sensors(void *dc, int first_row, int num_sensor, const int *dim, const int *stage, const int *norm, const double *norm_parameter,
                         const double *noise);
void mjpc_dc_set_process_noise(void *dc, const double *noise);
void mjpc_dc_set_mask(void *dc, const int *mask, int T);
void mjpc_dc_set_settings(void *dc, const int *flags, double timestep);
int mjpc_dc_assemble(void *dc, MjpcHipEngine *engine, int T, const double *residual_sensor, const double *residual_force, const double *DfDq,
                     const double *DfDv, const double *DfDa, const double *DsDq, const double *DsDv, const double *DsDa, const double *dvdq0,
                     const double *dvdq1);
/* the window the object owns, and its evaluation on the device: cost = DirectCost::Cost (nwin candidate windows in one
 * mjpc_hip_direct_cost call; q_windows NULL: the window itself; costs [nwin][3], failure [nwin][T]), cost_derivatives =
 * DirectCost::CostDerivatives (one mjpc_hip_direct_cost_derivatives call; the results through mjpc_dc_outputs, failure [T]) */
void mjpc_dc_set_window(void *dc, int T, int nq, int na, int nu, const double *q, const double *act, const double *ctrl, const double *time,
                        const double *sensor_measurement, const double *force_measurement);
void mjpc_dc_set_fd(void *dc, double tolerance, int mode, int discrete);
int mjpc_dc_cost(void *dc, MjpcHipEngine *engine, const double *q_windows, int nwin, const double *mocap, const double *userdata, double *costs,
                 int *failure);
int mjpc_dc_cost_derivatives(void *dc, MjpcHipEngine *engine, const double *mocap, const double *userdata, int *failure);
void mjpc_dc_outputs(void *dc, double *cost, double *gradient, double *hessian_band, double *block_sensor, double *block_force,
                     double *norm_gradient_sensor, double *norm_gradient_force, double *residual_sensor, double *residual_force);

/* CostDerivatives (mjpc/planners/cost_derivatives.h): create = Allocate + Reset; compute on the caller's engine under its current task.
 * 0 = ok, -1 = engine error (mjpc_hip_last_error). */
void *mjpc_cd_create(int dim_state_derivative, int dim_action, int dim_residual, int T);
void mjpc_cd_destroy(void *cd);
void mjpc_cd_reset(void *cd, int T);
int mjpc_cd_compute(void *cd, MjpcHipEngine *engine, const double *r, const double *rx, const double *ru, int T, int hessians);
/* the first T rows out of the object; any pointer may be NULL */
void mjpc_cd_blocks(void *cd, int T, double *cr, double *cx, double *cu, double *cxx, double *cuu, double *cxu);
/* Gradient::Compute (mjpc/planners/gradient/gradient.cc:43-108) on given arrays, host only (no GPU needed): A [T-1][nd][nd], B [T-1][nd][nu],
 * cx [T][nd], cu [T][nu] -> k [T][nu], Vx [T][nd], Qx [T-1][nd], Qu [T-1][nu], dV [2] (outputs may be NULL).  Returns the reference's
 * status (0 = complete); T < 2 goes through the error handler. */
int mjpc_gd_gradient_compute(int dim_state_derivative, int dim_action, int T, const double *A, const double *B, const double *cx, const double *cu,
                             double *k, double *Vx, double *Qx, double *Qu, double *dV);

/* GradientPlanner (mjpc/planners/gradient/planner.h): create = Initialize + Allocate.  representation 0 zero, 1 linear, 2 cubic; more than 25
 * spline points is refused through the error handler.  values out[6] = {action_step, expected, improvement, surprise, winner, failed};
 * timings out[5] = {nominal, derivatives, gradient (mapping), rollouts, policy update} in microseconds. */
void *mjpc_gd_create(const MjpcHipModel *model, const MjpcHipTask *task, int num_trajectory, int spline_points, int representation, int derivative_skip,
                     int max_rollout, double min_linesearch_step, double fd_tolerance, int fd_mode, int max_samples, int max_horizon, int device);
void mjpc_gd_destroy(void *planner);
void mjpc_gd_reset(void *planner, int horizon, const double *initial_repeated_action);
void mjpc_gd_set_state(void *planner, const double *state, const double *mocap, const double *userdata, double time);
void mjpc_gd_set_task(void *planner, const MjpcHipTask *task);
void mjpc_gd_set_num_trajectory(void *planner, int num_trajectory);
void mjpc_gd_optimize_policy(void *planner, int horizon);
void mjpc_gd_nominal_trajectory(void *planner, int horizon);
void mjpc_gd_action_from_policy(void *planner, double *action, double time, int use_previous);
double mjpc_gd_improvement(void *planner);
int mjpc_gd_policy(void *planner, double *times, double *values);                                  /* returns P */
void mjpc_gd_set_policy(void *planner, const double *times, const double *values);                 /* [P], [P][nu] */
int mjpc_gd_best_trajectory(void *planner, double *states, double *actions, double *costs, double *total_return);   /* returns H */
void mjpc_gd_values(void *planner, double *out);
void mjpc_gd_timings(void *planner, double *out);
void mjpc_gd_returns(void *planner, double *out, int n);          /* the last line search's returns */
int mjpc_gd_linesearch_steps(void *planner, double *out /* NULL: size only */);
int mjpc_gd_parameter_update(void *planner, double *out /* NULL: size only */);   /* M' k of the last iteration */
/* iLQGPlanner (mjpc/planners/ilqg/planner.h): create = Initialize + Allocate.  settings[9] = {min_linesearch_step, fd_tolerance, fd_mode,
 * min_regularization, max_regularization, regularization_type, max_regularization_iterations, action_limits, nominal_feedback_scaling}
 * (NULL: the reference's defaults); fused != 0: derivatives and backward pass in one device call.  values out[12] = {action_step, expected,
 * improvement, surprise, winner, backward pass failed, feedback_scaling, regularization, regularization_rate, all nominal rollouts failed,
 * dV[0], dV[1]}; timings out[6] = {nominal, derivatives + backward pass, rollouts, policy update (host, microseconds), resampling kernel,
 * rollout kernel (device, microseconds)}.  get_policy: which 0 policy, 1 previous_policy, 2 the nominal candidate; returns its horizon. */
void *mjpc_ilqg_create(const MjpcHipModel *model, const MjpcHipTask *task, int num_trajectory, int representation, int derivative_skip, int fused,
                       const double *settings, int max_samples, int max_horizon, int device);
void mjpc_ilqg_destroy(void *planner);
void mjpc_ilqg_reset(void *planner, int horizon, const double *initial_repeated_action);
void mjpc_ilqg_set_state(void *planner, const double *state, const double *mocap, const double *userdata, double time);
void mjpc_ilqg_set_task(void *planner, const MjpcHipTask *task);
void mjpc_ilqg_set_num_trajectory(void *planner, int num_trajectory);
void mjpc_ilqg_optimize_policy(void *planner, int horizon);
void mjpc_ilqg_nominal_trajectory(void *planner, int horizon);
void mjpc_ilqg_iteration(void *planner, int horizon);      /* only behind a nominal trajectory of the same horizon: refused otherwise */
void mjpc_ilqg_action_from_policy(void *planner, double *action, const double *state /* or NULL */, double time, int use_previous);
double mjpc_ilqg_improvement(void *planner);
int mjpc_ilqg_best_trajectory(void *planner, double *states, double *actions, double *costs, double *total_return);   /* returns H */
void mjpc_ilqg_values(void *planner, double *out);
void mjpc_ilqg_timings(void *planner, double *out);
void mjpc_ilqg_returns(void *planner, double *out, int n);
int mjpc_ilqg_linesearch_steps(void *planner, double *out /* NULL: size only */);
int mjpc_ilqg_get_policy(void *planner, int which, double *times, double *states, double *actions, double *feedback_gain, double *action_improvement,
                         double *feedback_scaling);
int mjpc_ilqg_best_rollout(const double *returns, const int *failures, int n);      /* iLQGPlanner::BestRollout, host only */
/* iLQSPlanner (mjpc/planners/ilqs/planner.h): create = Initialize + Allocate of a SamplingPlanner (exploration .. spline_points as for
 * mjpc_planner_create) and an iLQGPlanner (ilqg_num_trajectory .. settings as for mjpc_ilqg_create), each on its own engine.  Refused through
 * the error handler: spline_points < 2 or > 25, representation 0 (zero-order); the handle is then inert and only to be destroyed.
 * values out[6] = {active_policy, previous_active_policy (0 sampling, 1 iLQG), and of the last optimize_policy: converted iLQG's nominal to
 * a spline, returned early on sampling's improvement, ran an iLQG iteration, that iteration adopted a policy}; timings out[2] = {spline fit
 * of the last conversion (host, microseconds), 1 when it recomputed the cached operator}.  mjpc_ilqs_sampling / mjpc_ilqs_ilqg return BORROWED
 * handles for the mjpc_planner_* / mjpc_ilqg_* calls, owned by the iLQS planner: never destroy them. */
void *mjpc_ilqs_create(const MjpcHipModel *model, const MjpcHipTask *task, const double *exploration /* [2] */, int trajectories, int representation,
                       int sliding_plan, int spline_points, int ilqg_num_trajectory, int ilqg_representation, int derivative_skip, int fused,
                       const double *settings, int max_samples, int max_horizon, int device);
void mjpc_ilqs_destroy(void *planner);
void mjpc_ilqs_reset(void *planner, int horizon, const double *initial_repeated_action);
void mjpc_ilqs_set_state(void *planner, const double *state, const double *mocap, const double *userdata, double time);
void mjpc_ilqs_set_task(void *planner, const MjpcHipTask *task);
void mjpc_ilqs_optimize_policy(void *planner, int horizon);
void mjpc_ilqs_nominal_trajectory(void *planner, int horizon);
void mjpc_ilqs_action_from_policy(void *planner, double *action, const double *state /* or NULL; reaches iLQG only */, double time, int use_previous);
int mjpc_ilqs_best_trajectory(void *planner, double *states, double *actions, double *costs, double *total_return);   /* the active member's; returns H */
void mjpc_ilqs_values(void *planner, int *out);
void mjpc_ilqs_timings(void *planner, double *out);
void mjpc_ilqs_set_noise_exploration(void *planner, double first, double second);   /* sampling's GUI sliders noise_exploration[2] */
void *mjpc_ilqs_sampling(void *planner);
void *mjpc_ilqs_ilqg(void *planner);
int mjpc_ilqs_fitted_knots(void *planner, double *times, double *values);      /* the last conversion's knots, clamped: [P], [P][nu]; returns P */
/* sampling's batch member `index` of the last plan step (the reference's sampling.trajectory[index]); the planner's best trajectory is its
 * winner's again afterwards.  Any pointer may be NULL; returns H */
int mjpc_ilqs_sampling_member(void *planner, int index, double *states, double *actions, double *times, double *residual, double *total_return);
/* host closed forms without a planner (no GPU needed).  action_source: whose policy ActionFromPolicy evaluates, 0 sampling's current,
 * 1 sampling's previous, 2 iLQG's current, 3 iLQG's previous.  spline_fit: the least-squares knots out_knots [P][nu] of a spline
 * (representation 0 .. 2) over knot_times [P] through actions [H1][nu] at action_times [H1]; 0, or -1 when singular or out of range */
int mjpc_ilqs_action_source(int previous_active_policy, int active_policy, int use_previous);
int mjpc_ilqs_spline_fit(int representation, int P, const double *knot_times, int H1, const double *action_times, int nu, const double *actions,
                         double *out_knots);
/* host closed forms without a planner (no GPU needed): a spline mapping [(dim num_output)][(dim num_input)], GradientPolicy::Action */
void mjpc_gd_spline_mapping(int representation, int dim, const double *input_times, int num_input, const double *output_times, int num_output,
                            double *mapping);
void mjpc_gd_policy_action(int representation, int nu, const double *ctrlrange, const double *times, const double *parameters, int num_spline_points,
                           double time, double *action);

/* iLQGBackwardPass, BoxQP, iLQGPolicy (mjpc/planners/ilqg/): create = Allocate + Reset, with a BoxQP and the k / K rows of a policy inside.
 * Arrays as for mjpc_hip_ilqg_backward_pass (include/mjpc_hip.h): A [T-1][nd][nd], B [T-1][nd][nu], cx [T][nd], cu [T][nu], cxx [T][nd][nd],
 * cxu [T][nd][nu], cuu [T][nu][nu], actions [T-1][nu], action_limits [nu][2] (the two may be NULL without limits).  settings_i[3] =
 * {regularization_type, action_limits, max_regularization_iterations}, settings_d[2] = {min_regularization, max_regularization}; the
 * factor is the object's (2 after a reset).  k [T][nu], K [T][nu][nd] start as zeros; status[3] as the engine's.
 *   riccati_host     iLQGBackwardPass::RiccatiRegularized: the regularisation loop on the host (no GPU), bit-equal to the device
 *   riccati          iLQGBackwardPass::Riccati, the reference's signature: every sweep is handed `reg`; returns its status (0 = complete)
 *   compute          mjpc_hip_ilqg_backward_pass through iLQGBackwardPass::Compute; 0 = ok, -1 = engine error (mjpc_hip_last_error)
 *   compute_fused    mjpc_hip_trajectory_ilqg through ComputeFused: x [T][nq+nv+na], u [T][nu], h [T], residual [T][nr]; failure [T] */
void *mjpc_ilqg_bp_create(int dim_state_derivative, int dim_action, int T);
void mjpc_ilqg_bp_destroy(void *bp);
void mjpc_ilqg_bp_reset(void *bp, int T);
void mjpc_ilqg_bp_riccati_host(void *bp, int T, const double *A, const double *B, const double *cx, const double *cu, const double *cxx, const double *cxu,
                               const double *cuu, const double *actions, const double *action_limits, const int *settings_i, const double *settings_d,
                               double *k, double *K, int *status);
int mjpc_ilqg_bp_riccati(void *bp, int T, double reg, const double *A, const double *B, const double *cx, const double *cu, const double *cxx,
                         const double *cxu, const double *cuu, const double *actions, const double *action_limits, const int *settings_i,
                         const double *settings_d, double *k, double *K);
int mjpc_ilqg_bp_compute(void *bp, MjpcHipEngine *engine, int T, const double *A, const double *B, const double *cx, const double *cu, const double *cxx,
                         const double *cxu, const double *cuu, const double *actions, const double *action_limits, const int *settings_i,
                         const double *settings_d, double *k, double *K, int *status);
int mjpc_ilqg_bp_compute_fused(void *bp, MjpcHipEngine *engine, int T, const double *x, const double *u, const double *h, const double *residual,
                               const double *mocap, const double *userdata, double fd_tolerance, int fd_mode, const int *settings_i,
                               const double *settings_d, double *k, double *K, int *status, int *failure);
/* the first T rows out of the object (Q blocks: T - 1); any pointer may be NULL */
void mjpc_ilqg_bp_blocks(void *bp, int T, double *Vx, double *Vxx, double *Qx, double *Qu, double *Qxx, double *Qxu, double *Quu, double *dV);
/* {regularization, regularization_rate, regularization_factor}: set from `set` when not NULL, then read into `out` when not NULL */
void mjpc_ilqg_bp_regularization(void *bp, const double *set, double *out);
void mjpc_ilqg_bp_scale_regularization(void *bp, double factor, double reg_min, double reg_max);
void mjpc_ilqg_bp_update_regularization(void *bp, double reg_min, double reg_max, double z, double s);
/* BoxQPSolve (host, no GPU): res [n] warm start in, solution out; R [n][n] (its first nfree^2 entries: the factor of H_free), index [n];
 * lower / upper may be NULL.  Returns the number of free dimensions or -1. */
int mjpc_ilqg_boxqp(int n, const double *H, const double *g, const double *lower, const double *upper, double *res, double *R, int *index);
/* iLQGPolicy::Action (host, no GPU) of a policy given by its rows: times [horizon], states [horizon][nq+nv+na], actions [horizon][nu],
 * feedback_gain [horizon][nu][2nv+na]; the model's joint tables [njnt] and ctrlrange [nu][2]; state may be NULL (open loop) */
void mjpc_ilqg_policy_action(int nq, int nv, int na, int nu, int njnt, const int *jnt_type, const int *jnt_qposadr, const int *jnt_dofadr,
                             const double *ctrlrange, int representation, int horizon, const double *times, const double *states, const double *actions,
                             const double *feedback_gain, double feedback_scaling, const double *state, double time, double *action);

/* Kalman, Unscented (mjpc/estimators/; mjpc_hip::Kalman, mjpc_hip::Unscented of mjpc_hip_planner.h).  The engine is the caller's (created from the
 * same model and task with max_horizon >= 2) and outlives the estimator.  The measurement is residual rows [sensor_first_row, sensor_first_row +
 * num_sensor); `sensor` holds those num_sensor numbers.  settings[7] = {epsilon, flg_centered, alpha, beta, covariance_initial_scale,
 * process_noise_scale, sensor_noise_scale} or NULL for the defaults (1e-6, 0, 1, 2, 1e-4, 1e-4, 1e-4).  create returns NULL when the rows are not
 * inside the task's residual.  An update returns an EstimatorStatus: 0 ok, 1 covariance rank, 2 sensor-covariance rank, 3 a flagged step, 4 the
 * engine refused (mjpc_hip_last_error); on anything but 0 the state, covariance and time are what they were. */
void *mjpc_kalman_create(MjpcHipEngine *engine, const MjpcHipModel *model, const MjpcHipTask *task, int sensor_first_row, int num_sensor,
                         const double *settings);
void mjpc_kalman_destroy(void *estimator);
int mjpc_kalman_update_measurement(void *estimator, const double *ctrl, const double *sensor);
int mjpc_kalman_update_prediction(void *estimator);
int mjpc_kalman_update(void *estimator, const double *ctrl, const double *sensor);
void *mjpc_unscented_create(MjpcHipEngine *engine, const MjpcHipModel *model, const MjpcHipTask *task, int sensor_first_row, int num_sensor,
                            const double *settings);
void mjpc_unscented_destroy(void *estimator);
int mjpc_unscented_update(void *estimator, const double *ctrl, const double *sensor);
void mjpc_unscented_weights(void *estimator, double *out /* {sigma_step, weight_mean0, weight_covariance0, weight_sigma} */);
/* either kind.  dims out[4] = {nq+nv+na, nd, num_sensor, the engine's warning bits of the last update}; time: set from *set when not NULL, returned;
 * access: which 0 state [nq+nv+na], 1 covariance [nd][nd], 2 noise_process [nd], 3 noise_sensor [num_sensor]: set from `set` when not NULL, then
 * read into `out` when not NULL */
void mjpc_estimator_reset(void *estimator, const double *state, double time);
void mjpc_estimator_set_shared(void *estimator, const double *mocap, const double *userdata);
void mjpc_estimator_dims(void *estimator, int *out);
double mjpc_estimator_time(void *estimator, const double *set);
void mjpc_estimator_access(void *estimator, int which, const double *set, double *out);
/* the filter algebra as pure functions (host, no GPU; mjpc_hip_planner.h): row-major, a status other than 0 leaves the outputs untouched */
int mjpc_estimator_covariance_factor(int n, const double *P, double *L);
int mjpc_estimator_kalman_gain(int nd, int ns, const double *P, const double *C, const double *R, double *PCt, double *factor, double *gain);
void mjpc_estimator_kalman_correct(int nd, int ns, const double *PCt, const double *factor, const double *gain, const double *sensor_error,
                                   double *correction, double *P);
void mjpc_estimator_covariance_predict(int nd, const double *A, const double *Q, double *P);
int mjpc_estimator_unscented_correct(int nd, int ns, const double *cov_ss, const double *cov_sy, const double *cov_yy, const double *sensor_error,
                                     double *correction, double *P);

/* Closed-loop harness (include/mjpc_hip_testspeed.h; mjpc/testspeed.cc:44-129 `SynchronousPlanningCost`): world and planner on the
 * HIP engine.  planner_kind 0 = handle from mjpc_planner_create, 1 = handle from mjpc_cem_create, 2 = handle from mjpc_sg_create, 3 = handle from mjpc_gd_create, 4 = handle from mjpc_ilqg_create, 5 = handle from mjpc_ilqs_create (4 and 5: the policy is evaluated at the simulator's state).  state / mocap are in-out;
 * cost_per_step[ceil(total_time/timestep)] optional; out[6] = {average_cost, wall_seconds, realtime_factor, plan_seconds,
 * plan_steps, failure}.  Returns the total cost. */
double mjpc_testspeed_run(const MjpcHipModel *model, const MjpcHipTask *task, void *planner, int planner_kind, double *state,
                          double *mocap, double time0, int horizon, int steps_per_planning_iteration, double total_time, int device,
                          double *cost_per_step, double *out, int mode /* Task::mode */, double mode_time /* when the user selects it */,
                          double *task_parameters_out /* [num_parameter] or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* MJPC_HIP_PLANNER_C_H_ */
