// mjpc_hip_planner.h — C++ host side above the C ABI: the reference's SamplingPlanner surface, with the
// rollouts forwarded to the HIP engine (include/mjpc_hip.h).
//
// Mirrors (names, argument meaning, error behaviour):
//   mjpc/spline/spline.h:41-276              TimeSpline
//   mjpc/planners/sampling/policy.h,.cc      SamplingPolicy
//   mjpc/trajectory.h:74-86                  Trajectory (public arrays)
//   mjpc/planners/sampling/planner.h:51-162  SamplingPlanner (+ RankedPlanner virtuals, planners/planner.h:84-101)
//   mjpc/planners/cross_entropy/planner.h:32-147  CrossEntropyPlanner (same rollout engine, elite mean/variance update)
//   mjpc/planners/robust/robust_planner.h:31-80   RobustPlanner (top-k candidates x R noisy rollouts on a second engine)
//   mjpc/planners/sample_gradient/planner.h:35-175 SampleGradientPlanner (mixed batch; gradient reduced on the device)
//   mjpc/planners/model_derivatives.h:30-70  ModelDerivatives (finite-difference A, B, C, D along a trajectory, on the device)
//   mjpc/planners/cost_derivatives.h, planners/gradient/gradient.h  CostDerivatives (on the device), Gradient (backward recursion, host)
//   mjpc/planners/ilqs/planner.h             iLQSPlanner (a SamplingPlanner and an iLQGPlanner taking turns on one plan)
// Differences forced by the boundary: `mjModel*` / `const Task&` become the ABI's MjpcHipModel / MjpcHipTask views
// plus the planner's <custom><numeric> settings (Numerics); `ThreadPool&` arguments are gone (the GPU is the pool);
// `State` is passed as its raw arrays (State::CopyTo, mjpc/states/state.cc:128-135).
#ifndef MJPC_HIP_PLANNER_H_
#define MJPC_HIP_PLANNER_H_

#include <array>
#include <deque>
#include <shared_mutex>
#include <memory>
#include <vector>

#include "mjpc_hip.h"

namespace mjpc_hip {

inline constexpr int kMaxTrajectoryHorizon = 512;   // mjpc/trajectory.h:27
inline constexpr int MinSamplingSplinePoints = 1;    // mjpc/planners/sampling/planner.h:35-36
inline constexpr int MaxSamplingSplinePoints = 36;

enum SplineInterpolation : int { kZeroSpline = 0, kLinearSpline = 1, kCubicSpline = 2 };

// time-indexed spline of `dim`-vectors: zero / linear / cubic-Hermite sampling (spline.cc:103-156,240-277)
class TimeSpline {
 public:
  explicit TimeSpline(int dim = 0, SplineInterpolation interpolation = kZeroSpline, int initial_capacity = 1);
  std::size_t Size() const { return times_.size(); }
  int Dim() const { return dim_; }
  SplineInterpolation Interpolation() const { return interpolation_; }
  void SetInterpolation(SplineInterpolation interpolation) { interpolation_ = interpolation; }
  void Reserve(int num_nodes);
  void Sample(double time, double* values) const;             // values[dim]
  std::vector<double> Sample(double time) const;
  int DiscardBefore(double time);
  void Clear();
  double* AddNode(double time, const double* values = nullptr);   // returns the node's values; zeros when values == nullptr
  double NodeTime(int index) const { return times_[index]; }
  const double* NodeValues(int index) const { return values_[index].data(); }
  double* NodeValues(int index) { return values_[index].data(); }

 private:
  double Slope(int node_index, int value_index) const;
  SplineInterpolation interpolation_;
  int dim_;
  std::deque<double> times_;
  std::deque<std::vector<double>> values_;
};

// mjpc/planners/sampling/policy.cc:30-78
class SamplingPolicy {
 public:
  void Allocate(const MjpcHipModel* model, int num_spline_points);
  void Reset(int horizon, const double* initial_repeated_action = nullptr);
  void Action(double* action, const double* state, double time) const;     // spline sample, clamped to ctrlrange
  void CopyFrom(const SamplingPolicy& policy, int horizon);
  TimeSpline plan;
  int num_spline_points = 0;
  int nu = 0;
  std::vector<double> ctrlrange;
};

// mjpc/trajectory.h:74-86
struct Trajectory {
  int horizon = 0, dim_state = 0, dim_action = 0, dim_residual = 0, dim_trace = 0;
  std::vector<double> states, actions, times, residual, costs, trace;
  double total_return = 0;
  bool failure = false;
};

// configuration errors abort like mju_error (planner.cc:69-72) unless a handler is installed
void SetErrorHandler(void (*handler)(const char*));

struct Numerics {                       // the planner's <custom><numeric> entries (planner.cc:53-67, policy.cc:36-37)
  double sampling_exploration[2] = {0.1, 0.0};
  int sampling_trajectories = 10;
  int sampling_representation = kCubicSpline;
  int sampling_sliding_plan = 0;
  int sampling_spline_points = kMaxTrajectoryHorizon;
  int max_samples = 4096;              // kMaxTrajectory is 128 in the reference (planners/planner.h:28); lifted here
  double std_min = 0.1;                // cross-entropy: minimum std (cross_entropy/planner.cc:58)
  int robust_repetitions = 5;          // robust planner (robust_planner.cc:45-57)
  int robust_candidates = -1;          // default sampling_trajectories / robust_repetitions
  double robust_xfrc = 0.1, robust_xfrc_rate = 0.1;
  int n_elite = -1;                    // cross-entropy: default max(sampling_trajectories / 10, 2) (planner.cc:63-64)
  int max_horizon = kMaxTrajectoryHorizon;   // device trajectory buffers are sized max_samples x max_horizon
  int device = 0;                      // first HIP device ordinal
  int n_devices = 1;                   // SamplingPlanner: GPUs the candidate batch is sharded over (one engine each)
  std::vector<int> devices;            // optional explicit ordinals (repeats allowed); default device, device+1, ...
  int sample_gradient_trajectories = 0;    // sample gradient: gradient candidates among sampling_trajectories (sample_gradient/planner.cc:66)
  double sample_gradient_filter = 1.0;     // weight of the new gradient against the previous one (planner.cc:69)
  int gradient_num_trajectory = 32;        // gradient planner: line-search candidates (gradient/planner.cc:47)
  int gradient_spline_points = 10;         // policy knots; at most kMaxGradientSplinePoints (the reference's default, the horizon cap, overflows its own mapping)
  int gradient_representation = kLinearSpline;   // gradient/policy.cc:44-45
  int derivative_skip = 0;                 // knots left out between two evaluated ones (gradient/planner.cc:131)
};

// What the three planners on the rollout engine share: the planner's state, its policies, the bookkeeping of a plan step and the
// engine I/O around them.  Not polymorphic: nothing dispatches on a planner pointer, a planner is used as its own type.
class PlannerBase {
 public:
  PlannerBase() = default;
  PlannerBase(const PlannerBase&) = delete;
  PlannerBase& operator=(const PlannerBase&) = delete;

  void SetState(const double* state, const double* mocap, const double* userdata, double time);
  void ActionFromPolicy(double* action, const double* state, double time, bool use_previous = false);
  int NumParameters() { return policy.num_spline_points * nu_; }

  // ---- public members other code reads/writes in the reference (sampling/planner.h:115-162)
  SamplingPolicy policy, previous_policy;
  std::vector<double> state, mocap, userdata;
  double time = 0;
  std::vector<double> returns;                         // trajectory[i].total_return
  std::vector<int> failures;
  std::vector<int> trajectory_order;
  double improvement = 0;
  double noise_compute_time = 0, rollouts_compute_time = 0, policy_update_compute_time = 0;   // microseconds
  int interpolation_ = kZeroSpline;
  int num_trajectory_ = 10;
  unsigned long long seed = 0x5EED;
  unsigned long long plan_iter = 0;
  // reproducible-noise hook (the reference's absl::BitGen is unseedable): optional injected standard normals, one row of
  // P * nu per candidate of the batch
  const double* injected_noise_eps = nullptr;

 protected:
  ~PlannerBase() = default;
  // dimensions, ctrlrange_, num_trajectory_, interpolation_; false after the "Too many trajectories" refusal
  bool InitializeCommon(const MjpcHipModel* model, const MjpcHipTask* task, const Numerics& numerics);
  void AllocateState();                                // state / mocap / userdata, zeroed
  void ResetState(int horizon, const double* initial_repeated_action);   // state, time, policy, previous_policy
  void SizeTrajectory(Trajectory& trajectory) const;   // rows for numerics_.max_horizon steps
  // the spline's nodes as the ABI's knot arrays; returns their count.  An empty plan samples zeros: one knot at `time`.
  int KnotArrays(const TimeSpline& plan, std::vector<double>& times, std::vector<double>& values) const;
  // a plan of num_trajectory candidates at the current state / time; noise, explicit candidates, seed and stream are the caller's
  MjpcHipPlanInput PlanInput(const double* knot_times, const double* knot_values, int num_spline_points, int interpolation,
                             int num_trajectory, int horizon) const;
  static MjpcHipPlanOutput TrajectoryOutput(Trajectory& trajectory);   // the row pointers are the trajectory's buffers
  void OrderCandidates(int n);                         // trajectory_order[0 .. n) by (return, index)
  // `plan` alone, un-noised, on `engine` into `trajectory` (horizon, return and failure included; the engine's failure flags
  // into *failure); false after an engine error
  bool RolloutNominal(MjpcHipEngine* engine, const TimeSpline& plan, int horizon, Trajectory& trajectory, int* failure = nullptr);

  Numerics numerics_;
  int nq_ = 0, nv_ = 0, na_ = 0, ns_ = 0, nu_ = 0, nmocap_ = 0, nuserdata_ = 0, nr_ = 0, ntrace_ = 0;
  double timestep_ = 0;
  std::vector<double> ctrlrange_;
  mutable std::shared_mutex mtx_;
};

class SamplingPlanner : public PlannerBase {
 public:
  SamplingPlanner() { interpolation_ = kCubicSpline; }
  ~SamplingPlanner();

  // ---- Planner virtuals (planners/planner.h:38-80); errors abort like mju_error unless a handler is installed
  void Initialize(const MjpcHipModel* model, const MjpcHipTask* task, const Numerics& numerics);
  void Allocate();
  void Reset(int horizon, const double* initial_repeated_action = nullptr);
  void OptimizePolicy(int horizon);
  void NominalTrajectory(int horizon);
  const Trajectory* BestTrajectory();
  // ---- RankedPlanner virtuals (planners/planner.h:84-101)
  int OptimizePolicyCandidates(int ncandidates, int horizon);
  double CandidateScore(int candidate) const;
  void ActionFromCandidatePolicy(double* action, int candidate, const double* state, double time);
  void CopyCandidateToPolicy(int candidate);
  // ---- sampling-specific (planner.h:95-112)
  void UpdateNominalPolicy(int horizon);
  void SetTask(const MjpcHipTask* task);               // fresh ResidualFn copy per plan step (agent.cc:290)

  // knot values of candidate `candidate` (ranked order) of the last OptimizePolicyCandidates, [P*nu]; P via KnotTimes()
  void CandidateKnots(int candidate, double* out);
  // by batch index (unranked): the reference's trajectory[i] / candidate_policy[i] (ilqs/planner.cc:98-198); the rows land in
  // trajectory_winner
  void FetchCandidateUnranked(int index);
  void CandidateKnotsUnranked(int index, double* out);
  // every candidate's trace rows of the last plan step [num_trajectory][horizon][3*num_trace] in one copy (Traces, planner.cc:388-434)
  void AllTraces(double* out);
  const std::vector<double>& KnotTimes() const { return knot_times_; }
  Trajectory trajectory_winner;                        // trajectory[winner]; other candidates stay on the device
  int winner = 0;
  double noise_exploration[2] = {0.1, 0.0};
  int sliding_plan_ = 0;
  const int* injected_noise_sel = nullptr;             // [num_trajectory], with injected_noise_eps [num_trajectory * P * nu]

 private:
  void FetchCandidate(int global_index);
  MjpcHipMulti* engine_ = nullptr;             // one rollout engine per GPU
  SamplingPolicy winner_policy_;               // candidate_policy[winner]
  TimeSpline plan_scratch_;
  std::vector<double> knot_times_, knot_values_, winner_knots_;
  int last_horizon_ = 0, fetched_ = -1, nominal_horizon_ = 0;
  MjpcHipEngine* nominal_engine_ = nullptr;            // one-candidate engine of NominalTrajectory()
};

// mjpc/planners/cross_entropy/planner.{h,cc}: all N candidates are perturbed with a per-parameter std (elite variance,
// floored at std_min), the nominal (resampled) policy is rolled out as one extra candidate, the new policy is the mean
// of the n_elite best candidates.  Quirks kept: the variance loop reads the best elite's parameters for every elite
// (planner.cc:240-253); previous_policy is never refreshed by OptimizePolicy.
class CrossEntropyPlanner : public PlannerBase {
 public:
  CrossEntropyPlanner() = default;
  ~CrossEntropyPlanner();

  void Initialize(const MjpcHipModel* model, const MjpcHipTask* task, const Numerics& numerics);
  void Allocate();
  void Reset(int horizon, const double* initial_repeated_action = nullptr);
  void OptimizePolicy(int horizon);
  void NominalTrajectory(int horizon);
  void ResamplePolicy(int horizon);
  const Trajectory* BestTrajectory();                  // the nominal trajectory (planner.cc:418-420)
  void SetTask(const MjpcHipTask* task);

  SamplingPolicy resampled_policy;
  Trajectory nominal_trajectory;
  std::vector<double> parameters_scratch, times_scratch, variance;
  double std_initial_ = 0.1, std_min_ = 0.1;
  int n_elite_ = 2;
  // returns / failures: the candidates i < num_trajectory, then the nominal; injected_noise_eps: [(num_trajectory + 1) * P * nu]

 private:
  MjpcHipEngine* engine_ = nullptr;
  std::vector<double> knot_values_, noise_std_, all_knots_;
  int last_horizon_ = 0;
};

// mjpc/planners/robust/robust_planner.{h,cc}: the delegate ranks its candidates; the best `ncandidates_` are rolled out
// `nrepetitions_` times each with Ornstein-Uhlenbeck force noise on every body (Trajectory::NoisyRollout) in ONE launch of a
// second engine (explicit candidate policies); the candidate with the best mean return over the delegate's own score and
// its valid noisy rollouts is adopted.  The planner's state is the delegate's.
class RobustPlanner {
 public:
  RobustPlanner() = default;
  ~RobustPlanner();
  RobustPlanner(const RobustPlanner&) = delete;
  RobustPlanner& operator=(const RobustPlanner&) = delete;

  void Initialize(const MjpcHipModel* model, const MjpcHipTask* task, const Numerics& numerics);
  void Allocate() { delegate.Allocate(); }
  void Reset(int horizon, const double* initial_repeated_action = nullptr) { delegate.Reset(horizon, initial_repeated_action); }
  void SetState(const double* state, const double* mocap, const double* userdata, double time) { delegate.SetState(state, mocap, userdata, time); }
  void OptimizePolicy(int horizon);
  void NominalTrajectory(int horizon) { delegate.NominalTrajectory(horizon); }
  void ActionFromPolicy(double* action, const double* state, double time, bool use_previous = false) { delegate.ActionFromPolicy(action, state, time, use_previous); }
  const Trajectory* BestTrajectory() { return delegate.BestTrajectory(); }
  int NumParameters() { return delegate.NumParameters(); }
  void SetTask(const MjpcHipTask* task);

  SamplingPlanner delegate;                            // delegate_ (a RankedPlanner)
  int ncandidates_ = 12, nrepetitions_ = 5;
  double xfrc_std_ = 0.1, xfrc_rate_ = 0.1;
  std::vector<double> noisy_returns;                   // [ncandidates * nrepetitions] of the last OptimizePolicy
  std::vector<int> noisy_failures;
  std::vector<double> candidate_scores;                // mean score per candidate (robust_planner.cc:131-146)
  int best_candidate = -1;
  unsigned long long seed = 0x0B057;
  unsigned long long plan_iter = 0;

 private:
  MjpcHipEngine* engine_ = nullptr;                    // noisy rollouts (the delegate's engine keeps its plan for CopyCandidateToPolicy)
  Numerics numerics_;
  int nu_ = 0;
  std::vector<double> cand_knots_;
};

// mjpc/planners/sample_gradient/planner.{h,cc}: of the num_trajectory_ candidates of a plan step, candidate 0 is the (resampled)
// nominal, candidates 1 .. n_noisy-1 are nominal + noise_exploration * N(0, 1) (clamped), and the last num_gradient_ are policies
// the PREVIOUS plan step built along its gradient estimate; the best of all becomes the policy.  Then the noise of this step's
// noisy candidates, weighted by a fitness shaping of their returns, is summed into `gradient`, and num_gradient_ new candidates
// are laid along it at log-spaced step sizes for the next plan step.  One engine: the batch is one mjpc_hip_plan_mixed launch
// and the sum runs on the device over the engine's noise history (mjpc_hip_sample_gradient); no multi-GPU sharding.
// Restated formula by formula; the reference's quirks are kept:
//  - the noise is absolute: noise_exploration for every parameter, no ctrlrange scaling (planner.cc:346-351);
//  - num_gradient_ is clamped to num_trajectory - 1 on every call, and stays clamped (planner.cc:176);
//  - gradient candidates are host-side splines that persist between plans and are resampled to the current time by
//    ResamplePolicy before every plan, like the nominal (planner.cc:199-202); after Reset they are empty (all-zero actions);
//  - winner = order[0] only when its return is STRICTLY below the nominal's, else the nominal (planner.cc:232-237);
//  - previous_policy is never refreshed by OptimizePolicy;
//  - the return weights are computed once, when return_weight_.size() != n_noisy, and then cached for good: later plans reuse
//    the first plan's weights whatever the returns are (planner.cc:419-450);
//  - at that moment, and only then, the noisy candidates are re-sorted among themselves;
//  - the weights use log(trajectory_order[i] + 1): the candidate's INDEX, not its rank;
//  - on every other call the sum reads the first n_noisy entries of the order left by the full sort, which can name gradient
//    slots, whose noise history is zero or stale (planner.cc:454-459);
//  - the history keeps stale values in slot 0, the explicit slots and behind P * nu when the sliders move (include/mjpc_hip.h);
//  - the step sizes are cached on their count (utilities.cc:802-808 LogScale(2.0, 1e-3)); their first value is pinned to 1e-3
//    exactly (the reference's exp(log(1e-3)) is one ulp above it with glibc), the others are the reference's expression;
//  - gradient_previous enters un-resampled (planner.cc:486).
// Deliberate difference: std::partial_sort is not stable; candidates are ordered by (return, index), lowest index first, as
// everywhere in this repository (failed candidates all tie at 1e6).  All candidates of a plan share one interpolation.
class SampleGradientPlanner : public PlannerBase {
 public:
  enum WinnerType : int { kNominal = 0, kPerturb, kGradient };
  SampleGradientPlanner() = default;
  ~SampleGradientPlanner();

  void Initialize(const MjpcHipModel* model, const MjpcHipTask* task, const Numerics& numerics);
  void Allocate();
  void Reset(int horizon, const double* initial_repeated_action = nullptr);
  void OptimizePolicy(int horizon);
  void NominalTrajectory(int horizon);                 // rolls resampled_policy out into trajectory[0] (planner.cc:276-287)
  void ResamplePolicy(SamplingPolicy& policy, int horizon, int num_spline_points);
  const Trajectory* BestTrajectory();                  // trajectory[winner]
  void SetTask(const MjpcHipTask* task);
  // candidate_policy[index] as the reference holds it after OptimizePolicy: the rolled-out knots for index < n_noisy, the
  // freshly built gradient candidate otherwise; returns P, fills times[P] / values[P * nu] when non-null
  int CandidatePolicy(int index, double* times, double* values);
  // host closed forms (static: the tests call them without an engine)
  static void ReturnWeights(const int* order, int num_noisy, double* weights);      // planner.cc:437-449
  static void LogScale(double* values, double max_value, double min_value, int steps);   // utilities.cc:802-808

  SamplingPolicy resampled_policy;
  Trajectory trajectory_winner;                        // trajectory[winner]; the other candidates stay on the device
  double noise_exploration = 0.1;
  int num_gradient_ = 0;
  double gradient_filter_ = 1.0;
  std::vector<double> gradient, gradient_previous;     // [max spline points * nu]
  std::vector<double> step_size_;
  double gradient_max_step_size = 2.0, gradient_min_step_size = 1.0e-3;
  std::vector<double> return_weight_;
  int winner = 0;
  int winner_type_ = kNominal;
  double gradient_candidates_compute_time = 0;         // microseconds

 private:
  void GradientCandidates(int num_trajectory, int num_gradient, int horizon);
  SamplingPolicy& Candidate(int index);                // candidate_policy[index], materialised from the last plan's knots on demand
  MjpcHipEngine* engine_ = nullptr;
  std::vector<double> knot_times_, knot_values_, noise_std_, cand_table_, all_knots_, scale_;
  std::vector<SamplingPolicy> candidate_policy_;       // explicit (gradient) candidates; noisy ones live in all_knots_
  std::vector<char> candidate_valid_;                  // candidate_policy_[i] is current (else: row i of all_knots_ / empty)
  int last_horizon_ = 0, last_N_ = 0, last_P_ = 0, last_interp_ = kZeroSpline;
  TimeSpline plan_scratch_;
};

// mjpc/planners/model_derivatives.{h,cc}: transition and sensor (residual) Jacobians along a nominal trajectory, what iLQG, the
// gradient planner and iLQS linearise around.  The reference runs one mjd_transitionFD per evaluated knot on its thread pool;
// here the evaluated knots go to the device in ONE mjpc_hip_transition_fd call (gathered rows) and the rest is interpolated on
// the host with the reference's weights.  Blocks are row-major per knot: A[t] is [nd][nd], B[t] [nd][nu], C[t] [nr][nd],
// D[t] [nr][nu] (nd = dim_state_derivative, nr = dim_sensor = the task's num_residual; the definition of the entries is
// mjpc_hip_transition_fd's, include/mjpc_hip.h).  Index T - 1 is the terminal knot: C only, its A / B / D stay zero.
class ModelDerivatives {
 public:
  // dim_state = nq + nv + na, the row length of Compute's x (the reference passes it to Compute; here it is set once)
  void Allocate(int dim_state_derivative, int dim_action, int dim_sensor, int T, int dim_state = 0);
  void Reset(int dim_state_derivative, int dim_action, int dim_sensor, int T);    // zero the first T blocks
  // x [T][dim_state], u [T][dim_action], h [T] = the knots' times; tol = the finite-difference eps, mode = mjd_transitionFD's
  // flg_centered, skip = knots left out between two evaluated ones.  mocap / userdata are those of the planner's state.  T < 2 is an
  // error; false after an engine error (mjpc_hip_last_error).
  bool Compute(MjpcHipEngine* engine, const double* x, const double* u, const double* h, int T, double tol, int mode, int skip,
               const double* mocap = nullptr, const double* userdata = nullptr);
  // the two halves of Compute without an engine: the reference's evaluate_ / interpolate_ index sets (an index it lists twice
  // appears once), and every interpolated block from the evaluated ones, (1 - tt) L + tt U formed as mju_scl then mju_addToScl
  void IndexSets(int T, int skip);
  void Interpolate();

  std::vector<double> A, B, C, D;
  std::vector<int> failure;                            // [T]: MJPC_WARN_* bits of the evaluations at an evaluated knot, 0 elsewhere
  std::vector<int> evaluate_, interpolate_;
  int dim_state = 0, dim_state_derivative = 0, dim_action = 0, dim_sensor = 0;

 private:
  std::vector<double> gx_, gu_, gh_, gA_, gB_, gC_, gD_;
  std::vector<int> gfail_;
};

// mjpc/direct/direct.cc:1641-1830 (Direct::InverseDynamicsDerivatives): the Jacobians of the inverse dynamics f = qfrc_inverse and of
// the sensors s = the task's residual with respect to configuration, velocity and acceleration along a window of T configurations,
// what the direct optimiser and the batch estimator linearise around.  The reference runs one mjd_inverseFD per configuration on its
// thread pool; here the window goes to the device in ONE mjpc_hip_inverse_fd call.  Blocks are row-major per configuration and NOT
// transposed: DfDq[t] is [nv][nv] with entry [i][j] = d f_i / d q_j, DsDq[t] is [nr][nv] (direct.cc transposes mjd_inverseFD's
// output into this form).  The ends of the window follow the reference:
//   t = 0      evaluated at zero velocity and acceleration; only DsDq is kept, and of it only the position-stage rows
//   t = T - 1  evaluated at zero acceleration; only DsDq and DsDv are kept, and of them not the acceleration-stage rows
// Every other block of the two ends is zero (the device computes all six blocks for every configuration and the ends are zeroed on the
// host afterwards: the reference passes NULL for the blocks it drops there, so 2 of T configurations do some unused work in exchange for
// one call).  The stage of a residual row (the reference's sensor_needstage) comes from the task's
// table (RowStagesFromTable); rows of a task without a table count as acceleration stage.
class InverseDerivatives {
 public:
  enum { kStagePos = 0, kStageVel = 1, kStageAcc = 2 };
  void Allocate(int dim_state /* nq + nv + na */, int nq, int nv, int dim_action, int dim_sensor, int T);
  void Reset(int T);                                   // zero the first T blocks
  void SetRowStages(const int* stage);                 // [dim_sensor] of kStage*; Allocate sets every row to kStageAcc
  // the stages of a MJPC_TASK_TABLE residual: a block takes the latest stage among its terms (velocities: kStageVel; actuator forces
  // and every late kind: kStageAcc).  false (and nothing written) when the task is not a table
  static bool RowStagesFromTable(const MjpcHipTask* task, int* stage);
  // x [T][dim_state], u [T][dim_action], a [T][nv], h [T] = the configurations' times; tol = the finite-difference eps, mode =
  // flg_centered, discrete = mjENBL_INVDISCRETE.  T < 1 is an error; false after an engine error (mjpc_hip_last_error)
  bool Compute(MjpcHipEngine* engine, const double* x, const double* u, const double* a, const double* h, int T, double tol, int mode, int discrete,
               const double* mocap = nullptr, const double* userdata = nullptr);

  std::vector<double> DfDq, DfDv, DfDa, DsDq, DsDv, DsDa;
  std::vector<int> failure;                            // [T]: MJPC_WARN_* bits of the evaluations at t
  std::vector<int> row_stage;                          // [dim_sensor]
  int dim_state = 0, dim_q = 0, dim_v = 0, dim_action = 0, dim_sensor = 0;

 private:
  std::vector<double> gx_, ga_;
};

// mjpc/direct/direct.cc:683-1480, 1945-2106 (Direct::Cost with gradient and Hessian, from BlockSensor / BlockForce to TotalHessian): the
// cost of a window of T >= 3 configurations, its gradient [nv T] and its Gauss-Newton Hessian in MuJoCo's lower band [nv T][3 nv],
// from the residuals, the six blocks of InverseDerivatives and the velocity blocks dv_t/dq_{t-1}, dv_t/dq_t.  The formulas, the layout
// and the order of every sum are those of mjpc_hip_direct_assemble (include/mjpc_hip.h).  Assemble runs them on the device;
// AssembleHost is the same algebra on the host by the same summation rule (this library is compiled without contraction) and gives
// the device's bits, as Gradient and iLQGBackwardPass give theirs'.  The sensors are runs of rows of the engine's residual.
// Cost and CostDerivatives evaluate the window it owns on the device (mjpc_hip_direct_cost, mjpc_hip_direct_cost_derivatives).
// Not here yet: the band solve and the optimiser's loop.
class DirectCost {
 public:
  enum { kStagePos = 0, kStageVel = 1, kStageAcc = 2 };
  struct Settings {            // direct.h's defaults
    bool sensor_flag = true, force_flag = true, time_scaling_sensor = true, time_scaling_force = true;
    bool first_step_position_sensors = true, last_step_position_sensors = false, last_step_velocity_sensors = false;
  } settings;
  double timestep = 0.0;

  void Allocate(int nv, int nr, int T);                // noise_process = 1, no sensors, no mask
  // num_sensor sensors of dim[i] rows each, the first at residual row first_row; stage [num_sensor] of kStage*, norm [num_sensor] the cost
  // table's norm types, norm_parameter [num_sensor][2] = {p, q}, noise [num_sensor].  Clears the mask
  void SetSensors(int first_row, int num_sensor, const int* dim, const int* stage, const int* norm, const double* norm_parameter, const double* noise);
  void SetProcessNoise(const double* noise);           // [nv]
  void SetMask(const int* mask, int T);                // [T][num_sensor]; null: every sensor on
  // residual_sensor [T][ns], residual_force [T][nv], DfD* [T][nv][nv], DsD* [T][nr][nv], dvdq0, dvdq1 [T][nv][nv].  false after a
  // refusal (Assemble: mjpc_hip_last_error; AssembleHost refuses what the engine refuses, through the planner's error handler)
  bool Assemble(MjpcHipEngine* engine, int T, const double* residual_sensor, const double* residual_force, const double* DfDq, const double* DfDv,
                const double* DfDa, const double* DsDq, const double* DsDv, const double* DsDa, const double* dvdq0, const double* dvdq1);
  bool AssembleHost(int T, const double* residual_sensor, const double* residual_force, const double* DfDq, const double* DfDv, const double* DfDa,
                    const double* DsDq, const double* DsDv, const double* DsDa, const double* dvdq0, const double* dvdq1);

  // The window (Direct's configuration, act, ctrl, times, sensor_measurement, force_measurement) for Cost and CostDerivatives: T
  // configurations of the engine's model; act / ctrl / measurements null: zeros.  sensor_measurement [T][ns], force_measurement [T][nv]
  void SetWindow(int T, int nq, int na, int nu, const double* q, const double* act, const double* ctrl, const double* time,
                 const double* sensor_measurement, const double* force_measurement);
  double fd_tolerance = 1.0e-6;                        // finite-difference eps
  int fd_mode = 0, discrete = 1;                       // flg_centered, mjENBL_INVDISCRETE
  // the cost alone of nwin candidate windows q_windows [nwin][T][nq] (null: the window itself) in ONE mjpc_hip_direct_cost call, the
  // window's act, ctrl and measurements shared; costs [nwin][3].  false after an engine error (mjpc_hip_last_error)
  bool Cost(MjpcHipEngine* engine, const double* q_windows, int nwin, const double* mocap = nullptr, const double* userdata = nullptr);
  // cost, gradient, band Hessian and blocks of the window in ONE mjpc_hip_direct_cost_derivatives call, nothing downloaded in between
  bool CostDerivatives(MjpcHipEngine* engine, const double* mocap = nullptr, const double* userdata = nullptr);
  std::vector<double> configuration, act, ctrl, times, sensor_measurement, force_measurement;
  std::vector<double> costs;                           // [nwin][3] of the last Cost
  std::vector<int> failure;                            // [nwin][T] of the last Cost, [T] of the last CostDerivatives
  int window_length = 0, dim_q = 0, dim_act = 0, dim_action = 0;

  double cost[3] = {0.0, 0.0, 0.0};                    // cost, cost_sensor, cost_force
  std::vector<double> gradient, hessian_band;          // [nv T], [nv T][3 nv]
  std::vector<double> block_sensor, block_force;       // [T][ns][3 nv], [T][nv][3 nv]
  std::vector<double> norm_gradient_sensor, norm_gradient_force, residual_sensor, residual_force;      // [T][ns], [T][nv]
  std::vector<int> sensor_dim, sensor_stage, sensor_norm, sensor_mask;
  std::vector<double> sensor_norm_parameter, noise_sensor, noise_process;
  int dim_v = 0, dim_residual = 0, sensor_first_row = 0, num_sensor_rows = 0;

 private:
  void Size(int T);
  MjpcHipDirectSettings View(int T) const;
};

// mjpc/planners/cost_derivatives.{h,cc}: derivatives of the cost along a trajectory from the residual and its Jacobians.  The
// reference's third thread-pool fan-out (one task per knot) is ONE mjpc_hip_cost_derivatives call; the cost table and risk are the
// engine's current task, so Compute takes no norms / weights / parameters.  crr is not materialised (a dense type's Hessian is
// rebuilt from two scalars on the device).  Index T - 1 is the terminal knot: cx / cxx from rx alone, cu / cuu / cxu zero.
class CostDerivatives {
 public:
  void Allocate(int dim_state_derivative, int dim_action, int dim_residual, int T);
  void Reset(int dim_state_derivative, int dim_action, int dim_residual, int T);
  // r [T][nr], rx [T][nr][nd], ru [T][nr][nu]; hessians = false: cr, cx, cu only.  false after an engine error (mjpc_hip_last_error)
  bool Compute(MjpcHipEngine* engine, const double* r, const double* rx, const double* ru, int dim_state_derivative, int dim_action,
               int dim_residual, int T, bool hessians = true);

  std::vector<double> cr, cx, cu, cxx, cuu, cxu;
  int dim_state_derivative = 0, dim_action = 0, dim_residual = 0, horizon = 0;
};

// mjpc/planners/gradient/gradient.{h,cc}: the gradient planner's backward recursion over given model and cost derivatives, on the
// host, by the summation rule of mjpc_hip_cost_derivatives (include/mjpc_hip.h): bit-equal to the device's
// mjpc_hip_trajectory_gradient on the same matrices.  k [T][dim_action] stands in for GradientPolicy::k.
class Gradient {
 public:
  void Allocate(int dim_state_derivative, int dim_action, int T);
  void Reset(int dim_state_derivative, int dim_action, int T);
  // 0 = complete (the reference's return value); T < 2 is an error
  int Compute(double* k, const ModelDerivatives* md, const CostDerivatives* cd, int dim_state_derivative, int dim_action, int T);
  // the same over plain arrays: A [T-1][nd][nd], B [T-1][nd][nu], cx [T][nd], cu [T][nu]
  int Compute(double* k, const double* A, const double* B, const double* cx, const double* cu, int dim_state_derivative, int dim_action, int T);

  std::vector<double> Vx, Qx, Qu;                     // [T][nd], [T-1][nd], [T-1][nu]
  double dV[2] = {0.0, 0.0};
};

// ---- the gradient planner (mjpc/planners/gradient/): open-loop spline policy improved along the return's gradient
inline constexpr int kMaxGradientSplinePoints = 25;   // gradient/spline_mapping.h:27

// utilities.h:122-141, utilities.cc:286-404: the interval of `value` in an ascending sequence, and zero / linear / cubic interpolation of
// ys [length][dim] over xs (host arithmetic of GradientPolicy::Action; this library is compiled without contraction)
void FindInterval(int* bounds, const std::vector<double>& sequence, double value, int length);
void ZeroInterpolation(double* output, double x, const std::vector<double>& xs, const double* ys, int dim, int length);
void LinearInterpolation(double* output, double x, const std::vector<double>& xs, const double* ys, int dim, int length);
void CubicInterpolation(double* output, double x, const std::vector<double>& xs, const double* ys, int dim, int length);

// gradient/policy.{h,cc}
class GradientPolicy {
 public:
  void Allocate(const MjpcHipModel* model, const Numerics& numerics, int horizon);
  void Reset(int horizon, const double* initial_repeated_action = nullptr);
  void Action(double* action, const double* state, double time) const;     // FindInterval + interpolation, clamped to the ctrlrange
  void CopyFrom(const GradientPolicy& policy, int horizon);
  void CopyParametersFrom(const std::vector<double>& src_parameters, const std::vector<double>& src_times);

  std::vector<double> k;                  // action improvement [horizon][nu]
  std::vector<double> parameters, parameter_update, times;
  int num_parameters = 0, num_spline_points = 0, representation = kLinearSpline;
  int nu = 0;
  std::vector<double> ctrlrange;
};

// gradient/spline_mapping.{h,cc}: the linear operator from the policy's knot values [num_input][dim] to the actions at output_times
// [num_output][dim], row-major [(dim num_output)][(dim num_input)]
class SplineMapping {
 public:
  virtual ~SplineMapping() = default;
  virtual void Allocate(int dim);
  virtual void Compute(const std::vector<double>& input_times, int num_input, const double* output_times, int num_output) = 0;
  double* Get() { return mapping.data(); }
  int dim = 0;
  std::vector<double> mapping;
};
class ZeroSplineMapping : public SplineMapping {
 public:
  void Compute(const std::vector<double>& input_times, int num_input, const double* output_times, int num_output) override;
};
class LinearSplineMapping : public SplineMapping {
 public:
  void Compute(const std::vector<double>& input_times, int num_input, const double* output_times, int num_output) override;
};
class CubicSplineMapping : public SplineMapping {
 public:
  void Allocate(int dim) override;
  void Compute(const std::vector<double>& input_times, int num_input, const double* output_times, int num_output) override;
  std::vector<double> point_slope_mapping, output_mapping;
};

struct GradientPlannerSettings {          // gradient/settings.h
  int max_rollout = 1;                    // planner iterations per OptimizePolicy
  double min_linesearch_step = 1.0e-8;
  double fd_tolerance = 1.0e-5;
  int fd_mode = 0;                        // 0 one-sided, 1 centred
};

// gradient/planner.{h,cc}.  Stands alone (no SamplingPolicy members to carry).  One iteration: derivatives and gradient of the nominal
// trajectory (derivative_skip == 0: one mjpc_hip_trajectory_gradient; else ModelDerivatives, CostDerivatives, Gradient composed),
// parameter_update = M' k, num_trajectory candidates nominal + step_i * update at LogScale(1, min_linesearch_step) steps with the last
// step 0, rolled out as ONE explicit-candidate plan; the winner is picked on the host in the reference's order (j = N-1 .. 0, strict <
// against the best so far, starting from the nominal's return: a NaN return never wins) and fetched with mjpc_hip_get_candidate.
// Rollouts sample the knots with the engine's spline; ActionFromPolicy uses GradientPolicy::Action.  A failed derivative evaluation
// ends OptimizePolicy like gd_status != 0: the policy is left as it was (failed = true).
class GradientPlanner {
 public:
  GradientPlanner() = default;
  ~GradientPlanner();
  GradientPlanner(const GradientPlanner&) = delete;
  GradientPlanner& operator=(const GradientPlanner&) = delete;

  void Initialize(const MjpcHipModel* model, const MjpcHipTask* task, const Numerics& numerics);
  void Allocate();
  void Reset(int horizon, const double* initial_repeated_action = nullptr);
  void SetState(const double* state, const double* mocap, const double* userdata, double time);
  void SetTask(const MjpcHipTask* task);
  void OptimizePolicy(int horizon);
  void NominalTrajectory(int horizon);
  void ActionFromPolicy(double* action, const double* state, double time, bool use_previous = false);
  void ResamplePolicy(int horizon);
  const Trajectory* BestTrajectory() { return winner >= 0 ? &trajectory_winner : nullptr; }
  int NumParameters() { return policy.num_spline_points * nu_; }
  static void Refuse(const char* msg);                 // the planner error handler (abort unless one is installed)

  GradientPolicy policy, previous_policy, nominal_policy;      // nominal_policy: candidate_policy[0]
  GradientPlannerSettings settings;
  Gradient gradient;
  ModelDerivatives model_derivative;
  CostDerivatives cost_derivative;
  std::unique_ptr<SplineMapping> mappings[3];
  std::vector<double> state, mocap, userdata;
  double time = 0;
  std::vector<double> returns, linesearch_steps;       // of the last iteration
  std::vector<int> failures;
  Trajectory trajectory_nominal, trajectory_winner;
  int num_trajectory = 32, winner = -1, derivative_skip_ = 0;
  bool failed = false;                                 // the last OptimizePolicy stopped at a failed derivative
  double action_step = 0, expected = 0, improvement = 0, surprise = 0;
  double nominal_compute_time = 0, derivative_compute_time = 0, gradient_compute_time = 0, rollouts_compute_time = 0,
         policy_update_compute_time = 0;               // microseconds; derivative = model + cost (+ backward pass when fused)

 private:
  bool Rollout(const double* knots, int n, int horizon);       // n explicit candidates over nominal_policy.times -> returns / failures
  MjpcHipEngine* engine_ = nullptr;
  Numerics numerics_;
  int ns_ = 0, nd_ = 0, nu_ = 0, nr_ = 0, ntrace_ = 0, nmocap_ = 0, nuserdata_ = 0;
  double timestep_ = 0;
  std::vector<double> cand_knots_, parameters_scratch_, times_scratch_;
  mutable std::shared_mutex mtx_;
};

// ---- iLQG (mjpc/planners/ilqg/): boxqp.h, settings.h, policy.{h,cc}, backward_pass.{h,cc}, and the planner (iLQGPlanner, at the end of
// this header).  The components are the reference's public ones, which its iLQS (iLQSPlanner, below) drives as well.
// ilqg/boxqp.h: storage of the box-constrained control solve
class BoxQP {
 public:
  void Allocate(int n);
  std::vector<double> res, R, H, g, lower, upper;      // [n], [n][n], [n][n], [n], [n], [n]; res is the warm start and the solution
  std::vector<int> index;                              // [n] the free dimensions, ascending
};
// mju_boxQP's signature; MuJoCo is not part of this project: the method is defined in csrc/riccati.h (projected Newton; at most 100
// iterations, backtrack 0.5, Armijo 0.1, minimum step 1e-22, squared free gradient below 1e-16 stops) and restated here bit for bit.
// Returns the number of free dimensions (index lists them, R [nfree][nfree] row-major is the lower Cholesky factor of H_free), or -1
// when H_free is not positive definite.  lower / upper may be nullptr (unbounded).
int BoxQPSolve(double* res, double* R, int* index, const double* H, const double* g, int n, const double* lower, const double* upper);

struct iLQGSettings {                     // ilqg/settings.h
  double min_linesearch_step = 1.0e-3;
  double fd_tolerance = 1.0e-6;
  double fd_mode = 0;
  double min_regularization = 1.0e-6;
  double max_regularization = 1.0e6;
  int regularization_type = 0;           // 0: control; 1: feedback; 2: value; 3: none
  int max_regularization_iterations = 5;
  int action_limits = 1;
  int nominal_feedback_scaling = 1;
  int verbose = 0;
};
enum iLQGRegularizationType : int { kControlRegularization = 0, kStateControlRegularization, kValueRegularization, kNoRegularization };

// ilqg/policy.{h,cc}: time-varying affine feedback around a nominal trajectory
class iLQGPolicy {
 public:
  void Allocate(const MjpcHipModel* model, int num_residual, int num_trace, int horizon, int representation = kLinearSpline);
  // the same from the tables Action reads: dimensions, joint types / addresses (StateDiff), ctrlrange [nu][2]
  void Allocate(int nq, int nv, int na, int nu, int njnt, const int* jnt_type, const int* jnt_qposadr, const int* jnt_dofadr, const double* ctrlrange,
                int num_residual, int num_trace, int horizon, int representation = kLinearSpline);
  void Reset(int horizon, const double* initial_repeated_action = nullptr);
  // policy.cc:82-161: the interpolated nominal action, plus feedback_scaling * K (state (-) nominal state) when state != nullptr,
  // clamped to the ctrlrange.  The state difference is StateDiff (utilities.cc:525-535): for a ball or free joint's quaternion the
  // body-frame rotation vector of qa^-1 qb, the tangent of mjpc_hip_transition_fd.
  void Action(double* action, const double* state, double time) const;
  void CopyFrom(const iLQGPolicy& policy, int horizon);

  Trajectory trajectory;
  std::vector<double> feedback_gain;          // [horizon][nu][nd]
  std::vector<double> action_improvement;     // [horizon][nu]
  double feedback_scaling = 1.0;
  int representation = kLinearSpline;
  int nq = 0, nv = 0, na = 0, nu = 0;
  std::vector<double> ctrlrange;
  std::vector<int> jnt_type, jnt_qposadr, jnt_dofadr;

 private:
  mutable std::vector<double> state_scratch, action_scratch, feedback_gain_scratch, state_interp;
};
// utilities.cc:525-535 over the joint tables above: ds [2nv+na] = (s2 (-) s1) / h
// (the angle of a quaternion tangent comes from csrc/atan2_cr.h, a correctly rounded atan2 the feedback rollout kernel shares: DESIGN 8h)
void StateDiff(const iLQGPolicy& dims, double* ds, const double* s1, const double* s2, double h);

// ilqg/backward_pass.{h,cc}.  RiccatiStep and Riccati run on the host by the summation rule of csrc/riccati.h, bit-equal to the device's
// mjpc_hip_ilqg_backward_pass; Compute / ComputeFused run the device.
class iLQGBackwardPass {
 public:
  void Allocate(int dim_dstate, int dim_action, int T);
  void Reset(int dim_dstate, int dim_action, int T);
  // backward_pass.cc:65-250.  1 = ok, 0 = the control solve failed
  int RiccatiStep(int n, int m, double mu, const double* Wx, const double* Wxx, const double* At, const double* Bt, const double* cxt,
                  const double* cut, const double* cxxt, const double* cxut, const double* cuut, double* Vxt, double* Vxxt, double* dut,
                  double* Kt, double* dV, double* Qxt, double* Qut, double* Qxxt, double* Qxut, double* Quut, double* scratch, BoxQP& boxqp,
                  const double* action, const double* action_limits, int reg_type, int limits);
  // backward_pass.cc:253-324: 0 = complete, else the failing time index.  As in the reference, every retry is handed `reg`, not the
  // scaled member, and the box-QP's warm start is whatever boxqp.res holds.
  int Riccati(iLQGPolicy* p, const ModelDerivatives* md, const CostDerivatives* cd, int dim_dstate, int dim_action, int T, double reg,
              BoxQP& boxqp, const double* actions, const double* action_limits, const iLQGSettings& settings);
  // the regularisation loop of ilqg/planner.cc:429-520 on the host over plain arrays (the layout of mjpc_hip_ilqg_backward_pass), with
  // this object's regularization / regularization_rate: what the device kernel restates.  boxqp.res is zeroed first.  status [3].
  void RiccatiRegularized(double* k, double* K, const double* A, const double* B, const double* cx, const double* cu, const double* cxx,
                          const double* cxu, const double* cuu, int dim_dstate, int dim_action, int T, BoxQP& boxqp, const double* actions,
                          const double* action_limits, const iLQGSettings& settings, int* status);
  // the same on the device, into policy->action_improvement / feedback_gain and this object's blocks.  false after an engine error.
  bool Compute(MjpcHipEngine* engine, iLQGPolicy* policy, const ModelDerivatives* md, const CostDerivatives* cd, int dim_dstate, int dim_action,
               int T, const double* actions, const double* action_limits, const iLQGSettings& settings, int* status);
  // mjpc_hip_trajectory_ilqg: derivatives and backward pass in one call (x, u, h as for ModelDerivatives::Compute; residual [T][nr])
  bool ComputeFused(MjpcHipEngine* engine, iLQGPolicy* policy, const double* x, const double* u, const double* h, const double* residual,
                    int dim_dstate, int dim_action, int T, const iLQGSettings& settings, int* status, int* failure,
                    const double* mocap = nullptr, const double* userdata = nullptr);
  void ScaleRegularization(double factor, double reg_min, double reg_max);
  void UpdateRegularization(double reg_min, double reg_max, double z, double s);

  std::vector<double> Vx, Vxx, Qx, Qu, Qxx, Qxu, Quu, Q_scratch;
  double dV[2] = {0.0, 0.0};
  double regularization = 1.0, regularization_rate = 1.0, regularization_factor = 2.0;
};

// ilqg/planner.{h,cc}:156-223, 377-712 on one engine.  OptimizePolicy = NominalTrajectory + Iteration.
//  - NominalTrajectory: ONE mjpc_hip_plan_feedback in time mode over `policy` (FeedbackRollouts): candidate i has feedback scale
//    linesearch_steps[i] (LogScale(1, min_linesearch_step) with the last 0), no action step; the best rollout becomes candidate.trajectory
//    and feedback_scaling its step.  All candidates failed: candidate.trajectory = policy.trajectory, feedback_scaling = 0.
//  - Iteration: derivatives and backward pass of candidate.trajectory (fused: one mjpc_hip_trajectory_ilqg; composed: ModelDerivatives,
//    CostDerivatives, iLQGBackwardPass::Compute) into candidate's gains and improvement; a failed pass returns early, the policy unchanged.
//    ONE mjpc_hip_plan_feedback in indexed mode (ActionRollouts): action step linesearch_steps[i], feedback scale 1.  The winner is
//    picked on the host by BestRollout (from the last index down, strict <: the highest index wins a tie).  The adopted policy is the
//    reference's candidate_policy[winner]: gains and improvement of the pass, the NOMINAL's states, actions ubar + step k (unclamped) -
//    except for winner 0, whose slot the reference has by then overwritten with the winning rollout itself (planner.cc:561 before :596).
//    previous_policy = policy; policy.feedback_scaling = 1.
constexpr int kMaxiLQGTrajectory = 128;        // kMaxTrajectory (planners/planner.h:28): the reference's cap on the batch
class iLQGPlanner {
 public:
  iLQGPlanner() = default;
  ~iLQGPlanner();
  iLQGPlanner(const iLQGPlanner&) = delete;
  iLQGPlanner& operator=(const iLQGPlanner&) = delete;

  void Initialize(const MjpcHipModel* model, const MjpcHipTask* task, const Numerics& numerics);
  void Allocate();
  void Reset(int horizon, const double* initial_repeated_action = nullptr);
  void SetState(const double* state, const double* mocap, const double* userdata, double time);
  void SetTask(const MjpcHipTask* task);
  void OptimizePolicy(int horizon);
  bool NominalTrajectory(int horizon);                 // false: refused (horizon out of range, engine error); nothing was changed
  void Iteration(int horizon);                         // only behind a NominalTrajectory of the same horizon that returned true
  // iLQS's `candidate_policy[0].trajectory = sampling.trajectory[0]` (ilqs/planner.cc:198): the first `horizon` rows of `trajectory`
  // (states, actions, times, residual, costs), its return and failure flag become candidate.trajectory, the last action row repeating
  // the one before it as every rollout leaves it; linesearch_steps is sized for num_trajectory and Iteration(horizon) may follow.
  // false: refused (horizon out of range, dimensions that are not this planner's); nothing was changed
  bool SetNominal(const Trajectory& trajectory, int horizon);
  void ActionFromPolicy(double* action, const double* state, double time, bool use_previous = false);
  const Trajectory* BestTrajectory() { return winner >= 0 ? &trajectory_winner : nullptr; }
  // planner.cc:715-729: -1 when every candidate failed
  static int BestRollout(const double* returns, const int* failures, int n);
  static void LogScale(double* values, double max_value, double min_value, int steps);

  iLQGPolicy policy, previous_policy, candidate;       // candidate: candidate_policy[0]
  iLQGSettings settings;
  iLQGBackwardPass backward_pass;
  ModelDerivatives model_derivative;
  CostDerivatives cost_derivative;
  std::vector<double> state, mocap, userdata;
  double time = 0;
  std::vector<double> returns, linesearch_steps;       // of the last batch of rollouts
  std::vector<int> failures;
  Trajectory trajectory_winner;                        // the winning rollout of the last ActionRollouts
  int num_trajectory = 10;                             // ilqg_num_rollouts
  int representation = kLinearSpline;                  // ilqg_representation
  int winner = -1, derivative_skip_ = 0;
  bool fused = true;                                   // derivatives + backward pass in one device call (derivative_skip == 0 only)
  bool backward_pass_failed = false, all_failed = false;    // of the last OptimizePolicy
  bool adopted = false;                                // the last Iteration replaced `policy` (false: failed pass, every rollout failed, refusal)
  int backward_pass_status[3] = {0, 0, 0};
  double feedback_scaling = 1.0, action_step = 0, expected = 0, improvement = 0, surprise = 0;
  double nominal_compute_time = 0, derivative_compute_time = 0, rollouts_compute_time = 0, policy_update_compute_time = 0;   // microseconds
  double resample_kernel_time = 0, rollout_kernel_time = 0;       // device times of the last NominalTrajectory's resampling / last rollouts

 private:
  bool Rollouts(const iLQGPolicy& p, int mode, int horizon, const double* action_step, const double* feedback_scaling, bool use_feedback, bool improvement);
  bool Fetch(int index, int horizon, Trajectory& tr);
  MjpcHipEngine* engine_ = nullptr;
  Numerics numerics_;
  int ns_ = 0, nd_ = 0, nu_ = 0, nr_ = 0, ntrace_ = 0, nmocap_ = 0, nuserdata_ = 0;
  std::vector<double> ctrlrange_, zeros_, ones_;
  std::vector<int> fail_;
  bool nominal_ok_ = false; int nominal_horizon_ = 0;  // the last NominalTrajectory went through, at this horizon
  mutable std::shared_mutex mtx_;
};

// ---- iLQS (mjpc/planners/ilqs/planner.{h,cc}): sampling and iLQG taking turns on one plan.  A composition, as in the reference; each
// member keeps its own engine.  OptimizePolicy(horizon), ilqs/planner.cc:87-214:
//  1. previous_active_policy = active_policy;
//  2. if that is iLQG: ilqg.NominalTrajectory, then sampling.policy.plan becomes the P-knot spline fitted (SplineFit below) to the first
//     horizon - 1 actions of ilqg.candidate.trajectory, each knot clamped to the ctrlrange, at the times sampling.time + p time_shift
//     (repeated addition), time_shift = max((horizon - 1) timestep / (P - 1), 1e-5);
//  3. sampling.OptimizePolicy.  Kept from the reference: without sampling_sliding_plan its UpdateNominalPolicy rebuilds policy.plan from
//     the knots of sampling's own last winner, so the fitted plan of step 2 reaches the rollouts only with a sliding plan;
//  4. sampling improved when winner > 0 and returns[winner] < (previous was sampling ? returns[0] : ilqg.candidate's return), strictly:
//     active_policy = kSampling, iLQG's derivative / rollout / update timers are zeroed (the nominal one only when the active policy was
//     sampling already), return;
//  5. else, when the previous active policy was sampling, sampling's batch member 0 becomes iLQG's nominal (iLQGPlanner::SetNominal;
//     sampling.BestTrajectory() is its winner's again afterwards);
//  6. ilqg.Iteration;
//  7. if it adopted a policy and ilqg.trajectory_winner's return < (previous was sampling ? sampling.returns[winner] : ilqg.returns[0], the
//     full-step rollout of this iteration's batch), strictly: active_policy = kiLQG.
// Deliberate differences, where the reference is undefined:
//  - Initialize refuses sampling_spline_points < 2 (the reference divides by P - 1), > kMaxGradientSplinePoints (the mapping's capacity)
//    and sampling_representation == kZeroSpline (the last knot lies one step behind the last action: its column of the mapping is zero and
//    the normal matrix singular for every horizon and P);
//  - a fit whose normal matrix has a Cholesky pivot that is not positive and finite (linear with P >= horizon, for one) is refused,
//    "iLQS: spline fit is singular": the sampling plan stays as it was and OptimizePolicy returns;
//  - when ilqg.Iteration adopted nothing (failed backward pass, every rollout failed) active_policy stays: the reference would compare
//    returns left over from an earlier call.
// The mappings are allocated with dim = 1: the reference's [nu (H-1)][nu P] matrix is kron(M, I_nu), so the scalar M [H-1][P] is computed
// once and its pseudo-inverse W applied per actuator.  As in the reference, W is recomputed only when (H - 1, P) changed since the last
// conversion (here: or the representation); until then it belongs to the times of the conversion that filled it.
enum iLQSActivePolicy : int { kSampling = 0, kiLQG = 1 };

// W = (M'M)^-1 M' [P][H1] of M = mapping->Compute(knot_times, P, action_times, H1) [H1][P] (mapping->dim == 1): G = M'M, its lower
// Cholesky factor L (left-looking, row by row), then per column t of M' forward and back substitution.  Every sum starts at 0.0 and takes
// its index ascending, one rounded product and one rounded add per term (this library is compiled without contraction).  scratch is
// resized to P (P + 2).  Returns 0, or -1 when a pivot is not positive and finite (W is then unspecified).
int SplineFitOperator(SplineMapping* mapping, const std::vector<double>& knot_times, int P, const double* action_times, int H1, double* W,
                      std::vector<double>& scratch);
// knots [P][nu]: theta[p][j] = sum_t W[p][t] actions[t][j], by the same summation rule
void SplineFitApply(const double* W, int P, int H1, int nu, const double* actions, double* knots);
// both, without a cache: the least-squares knots of a `representation` spline over knot_times [P] through actions [H1][nu] at
// action_times [H1].  0, or -1: singular, representation not 0 .. 2, P not 1 .. kMaxGradientSplinePoints, H1 not 1 .. kMaxTrajectoryHorizon
int SplineFit(int representation, int P, const double* knot_times, int H1, const double* action_times, int nu, const double* actions,
              double* knots);

class iLQSPlanner {
 public:
  // whose Action ActionFromPolicy returns (ilqs/planner.cc:228-253)
  enum PolicySource : int { kSamplingCurrent = 0, kSamplingPrevious, kiLQGCurrent, kiLQGPrevious };
  iLQSPlanner();
  iLQSPlanner(const iLQSPlanner&) = delete;
  iLQSPlanner& operator=(const iLQSPlanner&) = delete;

  // ilqg.num_trajectory / representation / settings / fused are set on the member before Initialize, as for an iLQGPlanner
  void Initialize(const MjpcHipModel* model, const MjpcHipTask* task, const Numerics& numerics);
  void Allocate();
  void Reset(int horizon, const double* initial_repeated_action = nullptr);
  void SetState(const double* state, const double* mocap, const double* userdata, double time);
  void SetTask(const MjpcHipTask* task);
  void OptimizePolicy(int horizon);
  void NominalTrajectory(int horizon);
  void ActionFromPolicy(double* action, const double* state, double time, bool use_previous = false);   // state reaches iLQG only
  const Trajectory* BestTrajectory();
  // the four cases of use_previous: sampling's previous policy when it was active before; iLQG's CURRENT policy when iLQG was active
  // before and sampling returned early since (iLQG was not updated); iLQG's previous policy when it was updated
  static int ActionSource(int previous_active_policy, int active_policy, bool use_previous);

  SamplingPlanner sampling;
  iLQGPlanner ilqg;
  int active_policy = kSampling, previous_active_policy = kSampling;
  std::unique_ptr<SplineMapping> mappings[3];          // dim = 1
  std::vector<double> spline_times_cache, spline_parameters_cache;     // knot times [P], fitted and clamped knots [P][nu] of the last conversion
  std::vector<double> inversemapping;                  // W [P][H - 1]
  int dim_actions = 0, dim_parameters = 0, mapping_representation = -1;      // the cache key: H - 1, P, representation
  bool converted = false, returned_early = false, iterated = false;   // of the last OptimizePolicy
  bool fit_cache_miss = false;                         // the last conversion recomputed W
  double fit_compute_time = 0;                         // microseconds: mapping, factor and W when recomputed, and the product

 private:
  bool Convert(int horizon);                           // step 2 behind ilqg.NominalTrajectory; false: singular, the plan was left as it was
  bool initialized_ = false;
  int nu_ = 0;
  double timestep_ = 0;
  std::vector<double> ctrlrange_, fit_scratch_;
};

// ---- State estimators (mjpc/estimators/kalman.h, unscented.h) on the one-step engine -------------------------------------------
// The filter algebra is on the host, the model evaluations on the device: one mjpc_hip_linearize_step per EKF half-step, one
// mjpc_hip_unscented_moments per UKF update.  nd = 2nv+na.  The measurement is rows [sensor_first_row, sensor_first_row + ns) of the
// engine's residual (the reference's estimator_sensor_start); `sensor` arguments hold those ns numbers only.
//
// Failure policy, a deliberate deviation: the reference calls mju_error on a rank-deficient factor.  Here a rank-deficient covariance
// or sensor covariance, or a step the engine flagged, makes the update RETURN a status and leave state, covariance and time untouched.
enum EstimatorStatus : int {
  kEstimatorOk = 0,
  kEstimatorCovarianceRank = 1,    // the covariance has no Cholesky factor (a pivot is not > 0)
  kEstimatorSensorRank = 2,        // the sensor covariance C P C' + R, or cov_yy, has none
  kEstimatorStepFlagged = 3,       // the engine flagged an evaluation (MJPC_WARN_* bits in last_failure)
  kEstimatorEngineError = 4,       // the engine refused the call (mjpc_hip_last_error)
};

// The algebra as pure functions over row-major matrices.  Every contraction starts at 0.0 and runs over the ascending index with a
// rounded product and a rounded add per step; mju_symmetrize's rule is 0.5 * (m[i][j] + m[j][i]) for both entries.  A function that
// returns a status other than kEstimatorOk has written none of its outputs.
// lower Cholesky factor L [n][n] of P (zeros above the diagonal); false: a pivot is not > 0
bool CovarianceFactor(int n, const double* P, double* L);
// PCt [nd][ns] = P C', factor [ns][ns] = chol(C P C' + diag(R)), gain [nd][ns] with row i = (C P C' + R) \ PCt[i]  (kalman.cc:209-262)
int KalmanGain(int nd, int ns, const double* P, const double* C, const double* R, double* PCt, double* factor, double* gain);
// correction [nd] = PCt ((C P C' + R) \ sensor_error); P <- sym(P - PCt gain')  (kalman.cc:238-272)
void KalmanCorrect(int nd, int ns, const double* PCt, const double* factor, const double* gain, const double* sensor_error, double* correction,
                   double* P);
// P <- sym(A (P A') + diag(Q))  (kalman.cc:303-319)
void CovariancePredict(int nd, const double* A, const double* Q, double* P);
// correction [nd] = cov_sy (cov_yy \ sensor_error); P [nd][nd] = sym(cov_ss - cov_sy (cov_yy \ cov_sy')')  (unscented.cc:509-567)
int UnscentedCorrect(int nd, int ns, const double* cov_ss, const double* cov_sy, const double* cov_yy, const double* sensor_error,
                     double* correction, double* P);

struct EstimatorSettings {
  double epsilon = 1.0e-6;       // Kalman: finite-difference step
  bool flg_centered = false;     // Kalman: centred differences
  double alpha = 1.0, beta = 2.0;        // Unscented: sigma-point spread and prior knowledge (unscented.h defaults)
  // the reference's estimator_covariance_initial_scale, estimator_process_noise_scale, estimator_sensor_noise_scale numerics
  double covariance_initial_scale = 1.0e-4, process_noise_scale = 1.0e-4, sensor_noise_scale = 1.0e-4;
};

// what the two filters share: dimensions, the model's joint tables, the engine and the public estimate
class Estimator {
 public:
  // engine: created by the caller from the same model and task, with max_horizon >= 2; it stays the caller's.  0, or -1 when the
  // sensor rows are not inside the task's residual
  int Initialize(MjpcHipEngine* engine, const MjpcHipModel* model, const MjpcHipTask* task, int sensor_first_row, int num_sensor,
                 const EstimatorSettings& settings = EstimatorSettings());
  // covariance = scale I, the noises filled with their scales
  void Reset(const double* state, double time);
  void SetShared(const double* mocap, const double* userdata);      // what every evaluation sees beside state, ctrl and time
  // state <- state (+) correction: position integration over time 1 of correction[0:nv], a plain add on qvel and act
  void IntegrateState(double* state, const double* correction) const;

  std::vector<double> state, covariance, noise_process, noise_sensor;
  double time = 0.0;
  EstimatorSettings settings;
  int last_failure = 0;            // the engine's warning bits of the last update

  int nq = 0, nv = 0, na = 0, nu = 0, nr = 0, nd = 0, ns = 0, first = 0;
  double timestep = 0.0;

 protected:
  MjpcHipEngine* engine_ = nullptr;
  std::vector<int> jnt_type_, jnt_qposadr_, jnt_dofadr_;
  std::vector<double> mocap_, userdata_, ctrl_;
};

// mjpc/estimators/kalman.cc:188-330
class Kalman : public Estimator {
 public:
  int UpdateMeasurement(const double* ctrl, const double* sensor);     // EstimatorStatus
  int UpdatePrediction();                                              // under the last UpdateMeasurement's ctrl; advances time
  int Update(const double* ctrl, const double* sensor);                // both; a failed second half undoes the first
 private:
  std::vector<double> next_, residual_, A_, C_, PCt_, factor_, gain_, error_, correction_;
};

// mjpc/estimators/unscented.cc:484-574, weights :134-143
class Unscented : public Estimator {
 public:
  int Initialize(MjpcHipEngine* engine, const MjpcHipModel* model, const MjpcHipTask* task, int sensor_first_row, int num_sensor,
                 const EstimatorSettings& settings = EstimatorSettings());
  int Update(const double* ctrl, const double* sensor);                // EstimatorStatus; advances time
  double sigma_step = 0.0, weight_mean0 = 0.0, weight_covariance0 = 0.0, weight_sigma = 0.0;
  std::vector<double> sigma_next;      // [2nd+1][nq+nv+na]: the stepped sigma points of the last update
 private:
  std::vector<double> factor_, state_mean_, sensor_mean_, cov_ss_, cov_sy_, cov_yy_, error_, correction_, P_;
};

}  // namespace mjpc_hip
#endif  // MJPC_HIP_PLANNER_H_
