// planner.cc — C++ host side above the C ABI (include/mjpc_hip_planner.h) + a flat C wrapper for the tests.
// Restates, with the rollouts forwarded to the HIP engine:
//   mjpc/spline/spline.cc:103-277            TimeSpline::Sample / DiscardBefore / AddNode / Slope
//   mjpc/planners/sampling/policy.cc:30-78   SamplingPolicy
//   mjpc/planners/sampling/planner.cc:40-310,525-534   SamplingPlanner host logic
//   mjpc/planners/sample_gradient/planner.cc:43-493    SampleGradientPlanner host logic (batch + gradient sum on the engine)
//   mjpc/planners/model_derivatives.cc:24-165          ModelDerivatives (evaluations on the engine, interpolation on the host)
//   mjpc/planners/ilqg/backward_pass.cc, policy.cc, planner.cc:429-520   BoxQP, iLQGPolicy, iLQGBackwardPass (host, and the engine's kernel)
//   mjpc/planners/ilqs/planner.cc:33-263               iLQSPlanner (host; its spline fit is defined here, not MuJoCo's)
#include "../../include/mjpc_hip_planner.h"
#include "../../include/mjpc_hip_planner_c.h"
#include "atan2_cr.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <limits>
#include <numeric>

namespace mjpc_hip {

// ------------------------------------------------------------------ error convention
// The reference aborts through mju_error* on configuration errors (planner.cc:69-72); same here, unless a handler
// is installed (the Python tests install one that records the message instead of killing the interpreter).
static void (*g_error_handler)(const char*) = nullptr;
static void Fatal(const char* msg) {
  if (g_error_handler) { g_error_handler(msg); return; }
  std::fprintf(stderr, "mjpc_hip planner error: %s\n", msg);
  std::abort();
}

// ------------------------------------------------------------------ TimeSpline
TimeSpline::TimeSpline(int dim, SplineInterpolation interpolation, int) : interpolation_(interpolation), dim_(dim) {}
void TimeSpline::Reserve(int) {}
void TimeSpline::Clear() { times_.clear(); values_.clear(); }

double* TimeSpline::AddNode(double time, const double* new_values) {
  // spline.cc:203-238: only before the first or after the last node
  if (!(times_.empty() || time > times_.back() || time < times_.front())) {
    Fatal("Adding nodes to the middle of the spline isn't supported.");
    return nullptr;
  }
  std::vector<double> v(dim_, 0.0);
  if (new_values) std::copy(new_values, new_values + dim_, v.begin());
  if (times_.empty() || time > times_.back()) {
    times_.push_back(time); values_.push_back(std::move(v));
    return values_.back().data();
  }
  times_.push_front(time); values_.push_front(std::move(v));
  return values_.front().data();
}

int TimeSpline::DiscardBefore(double time) {   // spline.cc:164-188
  auto last_node = std::upper_bound(times_.begin(), times_.end(), time);
  if (last_node == times_.begin()) return 0;
  int keep_nodes = interpolation_ == kCubicSpline ? 1 : 0;
  last_node--;
  while (last_node != times_.begin() && keep_nodes) { last_node--; keep_nodes--; }
  int nodes_to_remove = (int)(last_node - times_.begin());
  times_.erase(times_.begin(), last_node);
  values_.erase(values_.begin(), values_.begin() + nodes_to_remove);
  return nodes_to_remove;
}

double TimeSpline::Slope(int node_index, int value_index) const {   // spline.cc:259-277
  if (node_index == 0)
    return (values_[1][value_index] - values_[0][value_index]) / (times_[1] - times_[0]);
  if (node_index == (int)times_.size() - 1)
    return (values_[node_index][value_index] - values_[node_index - 1][value_index]) / (times_[node_index] - times_[node_index - 1]);
  return 0.5 * (values_[node_index + 1][value_index] - values_[node_index][value_index]) / (times_[node_index + 1] - times_[node_index]) +
         0.5 * (values_[node_index][value_index] - values_[node_index - 1][value_index]) / (times_[node_index] - times_[node_index - 1]);
}

void TimeSpline::Sample(double time, double* values) const {   // spline.cc:103-156
  if (times_.empty()) { std::fill(values, values + dim_, 0.0); return; }
  auto upper = std::upper_bound(times_.begin(), times_.end(), time);
  if (upper == times_.end()) { const auto& n = values_[times_.size() - 1]; std::copy(n.begin(), n.end(), values); return; }
  if (upper == times_.begin()) { const auto& n = values_[0]; std::copy(n.begin(), n.end(), values); return; }
  int iu = (int)(upper - times_.begin()), il = iu - 1;
  double lo = times_[il], up = times_[iu];
  double t = (time - lo) / (up - lo);
  const auto& lower_node = values_[il];
  const auto& upper_node = values_[iu];
  switch (interpolation_) {
    case kZeroSpline:
      std::copy(lower_node.begin(), lower_node.end(), values);
      return;
    case kLinearSpline:
      for (int i = 0; i < dim_; i++) values[i] = lower_node[i] * (1 - t) + upper_node[i] * t;
      return;
    case kCubicSpline: {
      double c0 = 2.0 * t*t*t - 3.0 * t*t + 1.0;
      double c1 = (t*t*t - 2.0 * t*t + t) * (up - lo);
      double c2 = -2.0 * t*t*t + 3 * t*t;
      double c3 = (t*t*t - t*t) * (up - lo);
      for (int i = 0; i < dim_; i++) {
        double p0 = lower_node[i], m0 = Slope(il, i), m1 = Slope(iu, i), p1 = upper_node[i];
        values[i] = c0 * p0 + c1 * m0 + c2 * p1 + c3 * m1;
      }
      return;
    }
    default:
      Fatal("Unknown interpolation");
  }
}
std::vector<double> TimeSpline::Sample(double time) const {
  std::vector<double> v(dim_);
  Sample(time, v.data());
  return v;
}

// ------------------------------------------------------------------ SamplingPolicy
void SamplingPolicy::Allocate(const MjpcHipModel* model, int nsp) {
  nu = model->nu;
  ctrlrange.assign(model->actuator_ctrlrange, model->actuator_ctrlrange + 2 * nu);
  num_spline_points = nsp;
  plan = TimeSpline(nu);
}
void SamplingPolicy::Reset(int, const double* initial_repeated_action) {
  plan.Clear();
  if (initial_repeated_action != nullptr) plan.AddNode(0, initial_repeated_action);
}
void SamplingPolicy::Action(double* action, const double*, double time) const {
  if (action == nullptr) { Fatal("SamplingPolicy::Action: action == nullptr"); return; }
  plan.Sample(time, action);
  for (int i = 0; i < nu; i++) action[i] = std::max(ctrlrange[2 * i], std::min(ctrlrange[2 * i + 1], action[i]));   // Clamp
}
void SamplingPolicy::CopyFrom(const SamplingPolicy& p, int) {
  plan = p.plan; num_spline_points = p.num_spline_points; nu = p.nu; ctrlrange = p.ctrlrange;
}
// the policy's knots for the flat C view: returns P; fills times[P] and values[P * nu] when non-null
static int CopyKnots(const SamplingPolicy& policy, double* times, double* values) {
  int P = (int)policy.plan.Size();
  for (int i = 0; i < P; i++) {
    if (times) times[i] = policy.plan.NodeTime(i);
    if (values) std::copy(policy.plan.NodeValues(i), policy.plan.NodeValues(i) + policy.nu, values + (size_t)i * policy.nu);
  }
  return P;
}

// ------------------------------------------------------------------ PlannerBase
static double Micros(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
}

// returns sorted ascending with every non-finite value treated as +inf: a strict weak order even when a rollout produced NaN
// (the engine's argmin skips NaN the same way)
static inline bool ReturnLess(double a, double b) {
  const double inf = std::numeric_limits<double>::infinity();
  if (!(a == a)) a = inf;
  if (!(b == b)) b = inf;
  return a < b;
}

// candidates 0 .. num_trajectory-1 of one plan on one engine; everything else (noise, explicit candidates, seed, stream) is zero
static MjpcHipPlanInput MakePlanInput(const double* state, const double* mocap, const double* userdata, double time,
                                      const double* knot_times, const double* knot_values, int num_spline_points, int interpolation,
                                      int num_trajectory, int horizon) {
  MjpcHipPlanInput in;
  std::memset(&in, 0, sizeof(in));
  in.state = state; in.mocap = mocap; in.userdata = userdata; in.time = time;
  in.knot_times = knot_times; in.knot_values = knot_values; in.num_spline_points = num_spline_points;
  in.interpolation = interpolation; in.num_trajectory = num_trajectory; in.horizon = horizon;
  in.candidate_offset = 0; in.num_local = num_trajectory;
  return in;
}

bool PlannerBase::InitializeCommon(const MjpcHipModel* model, const MjpcHipTask* task, const Numerics& numerics) {
  numerics_ = numerics;
  nq_ = model->nq; nv_ = model->nv; na_ = model->na; ns_ = nq_ + nv_ + na_; nu_ = model->nu; nmocap_ = model->nmocap; nuserdata_ = model->nuserdata;
  nr_ = task->num_residual; ntrace_ = task->num_trace; timestep_ = model->timestep;
  ctrlrange_.assign(model->actuator_ctrlrange, model->actuator_ctrlrange + 2 * nu_);
  num_trajectory_ = numerics.sampling_trajectories;
  interpolation_ = numerics.sampling_representation;
  if (num_trajectory_ > numerics.max_samples) {
    char msg[128]; std::snprintf(msg, sizeof(msg), "Too many trajectories, %d is the maximum allowed.", numerics.max_samples);
    Fatal(msg);
    return false;
  }
  return true;
}

void PlannerBase::AllocateState() { state.assign(ns_, 0.0); mocap.assign(7 * nmocap_, 0.0); userdata.assign(nuserdata_, 0.0); }

void PlannerBase::ResetState(int horizon, const double* initial_repeated_action) {
  std::fill(state.begin(), state.end(), 0.0); std::fill(mocap.begin(), mocap.end(), 0.0);
  std::fill(userdata.begin(), userdata.end(), 0.0);
  time = 0.0;
  policy.Reset(horizon, initial_repeated_action);
  previous_policy.Reset(horizon, initial_repeated_action);
}

void PlannerBase::SetState(const double* s, const double* m, const double* u, double t) {
  std::copy(s, s + ns_, state.begin());
  if (m) std::copy(m, m + 7 * nmocap_, mocap.begin());
  if (u) std::copy(u, u + nuserdata_, userdata.begin());
  time = t;
}

void PlannerBase::ActionFromPolicy(double* action, const double* s, double t, bool use_previous) {   // planner.cc:225-233
  const std::shared_lock<std::shared_mutex> lock(mtx_);
  if (use_previous) previous_policy.Action(action, s, t);
  else policy.Action(action, s, t);
}

void PlannerBase::SizeTrajectory(Trajectory& tr) const {
  size_t Hm = (size_t)numerics_.max_horizon;
  tr.dim_state = ns_; tr.dim_action = nu_; tr.dim_residual = nr_; tr.dim_trace = 3 * ntrace_;
  tr.states.assign(Hm * ns_, 0.0); tr.actions.assign(Hm * nu_, 0.0);
  tr.times.assign(Hm, 0.0); tr.residual.assign(Hm * nr_, 0.0);
  tr.costs.assign(Hm, 0.0); tr.trace.assign(Hm * 3 * std::max(ntrace_, 1), 0.0);
}

int PlannerBase::KnotArrays(const TimeSpline& plan, std::vector<double>& times, std::vector<double>& values) const {
  int P = (int)plan.Size();
  times.resize(std::max(P, 1)); values.resize((size_t)std::max(P, 1) * nu_);
  for (int p = 0; p < P; p++) {
    times[p] = plan.NodeTime(p);
    std::copy(plan.NodeValues(p), plan.NodeValues(p) + nu_, values.begin() + (size_t)p * nu_);
  }
  if (P == 0) { P = 1; times[0] = time; std::fill(values.begin(), values.end(), 0.0); }   // empty plan samples zeros
  return P;
}

MjpcHipPlanInput PlannerBase::PlanInput(const double* knot_times, const double* knot_values, int num_spline_points, int interpolation,
                                        int num_trajectory, int horizon) const {
  return MakePlanInput(state.data(), mocap.data(), userdata.data(), time, knot_times, knot_values, num_spline_points, interpolation,
                       num_trajectory, horizon);
}

MjpcHipPlanOutput PlannerBase::TrajectoryOutput(Trajectory& tr) {
  MjpcHipPlanOutput out;
  std::memset(&out, 0, sizeof(out));
  out.states = tr.states.data(); out.actions = tr.actions.data(); out.times = tr.times.data();
  out.residual = tr.residual.data(); out.costs = tr.costs.data(); out.trace = tr.trace.data();
  return out;
}

void PlannerBase::OrderCandidates(int n) {   // ties: lowest index, like the engine's argmin
  if ((int)trajectory_order.size() < n) trajectory_order.resize(n);
  std::iota(trajectory_order.begin(), trajectory_order.begin() + n, 0);
  std::stable_sort(trajectory_order.begin(), trajectory_order.begin() + n, [this](int a, int b) { return ReturnLess(returns[a], returns[b]); });
}

bool PlannerBase::RolloutNominal(MjpcHipEngine* engine, const TimeSpline& plan, int horizon, Trajectory& tr, int* failure) {
  std::vector<double> kt, kv;
  int P = KnotArrays(plan, kt, kv);
  MjpcHipPlanInput in = PlanInput(kt.data(), kv.data(), P, (int)plan.Interpolation(), 1, horizon);
  double ret = 0; int fail = 0;
  MjpcHipPlanOutput out = TrajectoryOutput(tr);
  out.returns = &ret; out.failure = &fail;
  if (mjpc_hip_plan(engine, &in, &out) != 0) { Fatal(mjpc_hip_last_error()); return false; }
  tr.horizon = horizon; tr.total_return = ret; tr.failure = fail != 0;
  if (failure) *failure = fail;
  return true;
}

// ------------------------------------------------------------------ SamplingPlanner
SamplingPlanner::~SamplingPlanner() {
  if (engine_) mjpc_hip_multi_destroy(engine_);
  if (nominal_engine_) mjpc_hip_destroy(nominal_engine_);
}

void SamplingPlanner::Initialize(const MjpcHipModel* model, const MjpcHipTask* task, const Numerics& numerics) {
  noise_exploration[0] = numerics.sampling_exploration[0];
  noise_exploration[1] = numerics.sampling_exploration[1];
  sliding_plan_ = numerics.sampling_sliding_plan;
  if (!InitializeCommon(model, task, numerics)) return;
  if (engine_) { mjpc_hip_multi_destroy(engine_); engine_ = nullptr; }     // the model might have changed
  // one engine per GPU (Numerics::n_devices, ordinals in Numerics::devices or device, device+1, ...): the candidate batch of a
  // plan step is block-partitioned over them (include/mjpc_hip.h, mjpc_hip_multi_plan)
  {
    int G = std::max(1, numerics.n_devices);
    std::vector<int> devs(G);
    for (int k = 0; k < G; k++) devs[k] = k < (int)numerics.devices.size() ? numerics.devices[k] : numerics.device + k;
    engine_ = mjpc_hip_multi_create(model, task, numerics.max_samples, numerics.max_horizon, G, devs.data());
  }
  if (!engine_) { Fatal(mjpc_hip_last_error()); return; }
  // NominalTrajectory() rolls the nominal policy out on its own one-candidate engine, so that the candidates of the last
  // plan step (returns, order, trajectories on the device) stay available to the RankedPlanner calls afterwards
  if (nominal_engine_) { mjpc_hip_destroy(nominal_engine_); nominal_engine_ = nullptr; }
  nominal_engine_ = mjpc_hip_create(model, task, 1, numerics.max_horizon, numerics.device);
  if (!nominal_engine_) { Fatal(mjpc_hip_last_error()); return; }
  policy.Allocate(model, numerics.sampling_spline_points);
  previous_policy.Allocate(model, numerics.sampling_spline_points);
  winner_policy_.Allocate(model, numerics.sampling_spline_points);
  winner = 0;
}

void SamplingPlanner::Allocate() {
  AllocateState();
  plan_scratch_ = TimeSpline(nu_);
  SizeTrajectory(trajectory_winner);
  returns.assign(numerics_.max_samples, 0.0); failures.assign(numerics_.max_samples, 0);
  winner = -1;
}

void SamplingPlanner::Reset(int horizon, const double* initial_repeated_action) {
  ResetState(horizon, initial_repeated_action);
  winner_policy_.Reset(horizon, initial_repeated_action);
  plan_scratch_.Clear();
  improvement = 0.0;
  winner = 0;
  fetched_ = -1;
}

void SamplingPlanner::SetTask(const MjpcHipTask* task) {
  if (mjpc_hip_multi_set_task(engine_, task) != 0) Fatal(mjpc_hip_last_error());
  if (nominal_engine_ && mjpc_hip_set_task(nominal_engine_, task) != 0) Fatal(mjpc_hip_last_error());
}

void SamplingPlanner::UpdateNominalPolicy(int horizon) {   // planner.cc:236-310
  int num_spline_points = winner_policy_.num_spline_points;
  double nominal_time = time;
  double time_horizon = (horizon - 1) * timestep_;
  if (sliding_plan_) {
    int extra_points = interpolation_ == kZeroSpline ? 1 : (interpolation_ == kLinearSpline ? 2 : 4);
    double time_shift;
    if (num_spline_points > extra_points) time_shift = std::max(time_horizon / (num_spline_points - extra_points), 1.0e-5);
    else time_shift = time_horizon;
    const std::unique_lock<std::shared_mutex> lock(mtx_);
    policy.plan.DiscardBefore(nominal_time);
    if (policy.plan.Size() == 0) policy.plan.AddNode(time);
    while ((int)policy.plan.Size() < num_spline_points) {
      int last = (int)policy.plan.Size() - 1;
      double new_node_time = policy.plan.NodeTime(last) + time_shift;
      std::vector<double> copy(policy.plan.NodeValues(last), policy.plan.NodeValues(last) + nu_);
      policy.plan.AddNode(new_node_time, copy.data());
    }
  } else {
    double time_shift;
    if (interpolation_ == kZeroSpline) time_shift = std::max(time_horizon / num_spline_points, 1.0e-5);
    else time_shift = std::max(time_horizon / (num_spline_points - 1), 1.0e-5);
    plan_scratch_.Clear();
    plan_scratch_.SetInterpolation((SplineInterpolation)interpolation_);
    for (int t = 0; t < num_spline_points; t++) {
      double* node = plan_scratch_.AddNode(nominal_time);
      winner_policy_.Action(node, nullptr, nominal_time);
      nominal_time += time_shift;                         // repeated addition, like the reference
    }
    const std::unique_lock<std::shared_mutex> lock(mtx_);
    policy.plan = plan_scratch_;
  }
}

int SamplingPlanner::OptimizePolicyCandidates(int ncandidates, int horizon) {   // planner.cc:151-187
  int num_trajectory = num_trajectory_;
  ncandidates = std::min(ncandidates, num_trajectory);
  auto rollouts_start = std::chrono::steady_clock::now();
  policy.plan.SetInterpolation((SplineInterpolation)interpolation_);
  int P = KnotArrays(policy.plan, knot_times_, knot_values_);
  winner_knots_.assign((size_t)P * nu_, 0.0);
  MjpcHipPlanInput in = PlanInput(knot_times_.data(), knot_values_.data(), P, interpolation_, num_trajectory, horizon);
  in.noise_exploration[0] = noise_exploration[0]; in.noise_exploration[1] = noise_exploration[1];
  in.noise_eps = injected_noise_eps; in.noise_sel = injected_noise_sel; in.seed = seed; in.stream = plan_iter++;
  MjpcHipPlanOutput out = TrajectoryOutput(trajectory_winner);
  out.returns = returns.data(); out.failure = failures.data(); out.winner_knots = winner_knots_.data();
  if (mjpc_hip_multi_plan(engine_, &in, &out) != 0) { Fatal(mjpc_hip_last_error()); return 0; }
  last_horizon_ = horizon; fetched_ = out.winner;
  noise_compute_time = out.noise_compute_time_us;
  // order so that the first ncandidates are the best
  trajectory_order.resize(num_trajectory);
  OrderCandidates(num_trajectory);
  rollouts_compute_time = Micros(rollouts_start);
  return ncandidates;
}

void SamplingPlanner::FetchCandidate(int global_index) {
  if (fetched_ == global_index) return;
  MjpcHipPlanOutput out = TrajectoryOutput(trajectory_winner);
  out.winner_knots = winner_knots_.data();
  if (mjpc_hip_multi_get_candidate(engine_, global_index, &out) != 0) { Fatal(mjpc_hip_last_error()); return; }
  fetched_ = global_index;
}

void SamplingPlanner::CopyCandidateToPolicy(int candidate) {   // planner.cc:525-534 (with a UNIQUE lock)
  winner = trajectory_order[candidate];
  FetchCandidate(winner);
  trajectory_winner.horizon = last_horizon_;
  trajectory_winner.total_return = returns[winner];
  trajectory_winner.failure = failures[winner] != 0;
  int P = (int)knot_times_.size();
  winner_policy_.plan = TimeSpline(nu_, (SplineInterpolation)interpolation_);
  for (int p = 0; p < P; p++) winner_policy_.plan.AddNode(knot_times_[p], winner_knots_.data() + (size_t)p * nu_);
  winner_policy_.num_spline_points = policy.num_spline_points;
  const std::unique_lock<std::shared_mutex> lock(mtx_);
  previous_policy.CopyFrom(policy, 0);
  policy.CopyFrom(winner_policy_, 0);
}

void SamplingPlanner::OptimizePolicy(int horizon) {   // planner.cc:190-208
  UpdateNominalPolicy(horizon);
  OptimizePolicyCandidates(1, horizon);
  auto policy_update_start = std::chrono::steady_clock::now();
  CopyCandidateToPolicy(0);
  double best_return = returns[0];
  improvement = std::max(best_return - returns[winner], 0.0);
  policy_update_compute_time = Micros(policy_update_start);
}

void SamplingPlanner::NominalTrajectory(int horizon) {   // planner.cc:211-222: rolls out `policy` into trajectory[0] only
  // one un-noised candidate on the dedicated engine: returns / failures / trajectory_order / candidate knots of the last
  // OptimizePolicyCandidates() are not touched (the reference writes nothing but trajectory[0] here either)
  policy.plan.SetInterpolation((SplineInterpolation)interpolation_);
  if (!RolloutNominal(nominal_engine_, policy.plan, horizon, trajectory_winner)) return;
  fetched_ = -1;                 // trajectory_winner no longer mirrors a candidate of the last plan: re-fetch on demand
  nominal_horizon_ = horizon;
  if (winner < 0) winner = 0;
}

const Trajectory* SamplingPlanner::BestTrajectory() { return winner >= 0 ? &trajectory_winner : nullptr; }

double SamplingPlanner::CandidateScore(int candidate) const { return returns[trajectory_order[candidate]]; }

void SamplingPlanner::ActionFromCandidatePolicy(double* action, int candidate, const double* s, double t) {
  FetchCandidate(trajectory_order[candidate]);
  TimeSpline sp(nu_, (SplineInterpolation)interpolation_);
  for (size_t p = 0; p < knot_times_.size(); p++) sp.AddNode(knot_times_[p], winner_knots_.data() + p * nu_);
  sp.Sample(t, action);
  for (int i = 0; i < nu_; i++) action[i] = std::max(ctrlrange_[2 * i], std::min(ctrlrange_[2 * i + 1], action[i]));
  (void)s;
}

// ------------------------------------------------------------------ CrossEntropyPlanner
CrossEntropyPlanner::~CrossEntropyPlanner() { if (engine_) mjpc_hip_destroy(engine_); }

void CrossEntropyPlanner::Initialize(const MjpcHipModel* model, const MjpcHipTask* task, const Numerics& numerics) {   // planner.cc:41-72
  std_initial_ = numerics.sampling_exploration[0];
  std_min_ = numerics.std_min;
  n_elite_ = numerics.n_elite > 0 ? numerics.n_elite : std::max(numerics.sampling_trajectories / 10, 2);
  if (!InitializeCommon(model, task, numerics)) return;
  if (engine_) { mjpc_hip_destroy(engine_); engine_ = nullptr; }
  engine_ = mjpc_hip_create(model, task, numerics.max_samples + 1, numerics.max_horizon, numerics.device);   // + the nominal rollout
  if (!engine_) { Fatal(mjpc_hip_last_error()); return; }
  policy.Allocate(model, numerics.sampling_spline_points);
  resampled_policy.Allocate(model, numerics.sampling_spline_points);
  previous_policy.Allocate(model, numerics.sampling_spline_points);
}

void CrossEntropyPlanner::Allocate() {   // planner.cc:75-117
  AllocateState();
  int P = policy.num_spline_points;
  parameters_scratch.assign((size_t)P * nu_, 0.0); times_scratch.assign(P, 0.0);
  variance.assign((size_t)P * nu_, 0.0); noise_std_.assign((size_t)P * nu_, 0.0); knot_values_.assign((size_t)P * nu_, 0.0);
  trajectory_order.resize(numerics_.max_samples);
  std::iota(trajectory_order.begin(), trajectory_order.end(), 0);
  returns.assign(numerics_.max_samples + 1, 0.0); failures.assign(numerics_.max_samples + 1, 0);
  SizeTrajectory(nominal_trajectory);
}

void CrossEntropyPlanner::Reset(int horizon, const double* initial_repeated_action) {   // planner.cc:120-155
  ResetState(horizon, initial_repeated_action);
  resampled_policy.Reset(horizon, initial_repeated_action);
  std::fill(parameters_scratch.begin(), parameters_scratch.end(), 0.0);
  std::fill(times_scratch.begin(), times_scratch.end(), 0.0);
  double var = std_initial_ * std_initial_;
  std::fill(variance.begin(), variance.end(), var);
  improvement = 0.0;
}

void CrossEntropyPlanner::SetTask(const MjpcHipTask* task) {
  if (mjpc_hip_set_task(engine_, task) != 0) Fatal(mjpc_hip_last_error());
}

void CrossEntropyPlanner::ResamplePolicy(int horizon) {   // planner.cc:313-338
  int num_spline_points = resampled_policy.num_spline_points;
  double nominal_time = time;
  double time_shift = std::max((horizon - 1) * timestep_ / (num_spline_points - 1), 1.0e-5);
  for (int t = 0; t < num_spline_points; t++) {
    times_scratch[t] = nominal_time;
    resampled_policy.Action(parameters_scratch.data() + (size_t)t * nu_, nullptr, nominal_time);
    nominal_time += time_shift;
  }
  SplineInterpolation keep = policy.plan.Interpolation();
  resampled_policy.plan.Clear();
  for (int t = 0; t < num_spline_points; t++) resampled_policy.plan.AddNode(times_scratch[t], parameters_scratch.data() + (size_t)t * nu_);
  resampled_policy.plan.SetInterpolation(keep);
}

void CrossEntropyPlanner::OptimizePolicy(int horizon) {   // planner.cc:164-283
  resampled_policy.plan.SetInterpolation((SplineInterpolation)interpolation_);
  int num_trajectory = num_trajectory_;
  n_elite_ = std::min(n_elite_, num_trajectory);
  int n_elite = std::min(n_elite_, num_trajectory);
  {
    const std::shared_lock<std::shared_mutex> lock(mtx_);
    resampled_policy.CopyFrom(policy, policy.num_spline_points);
  }
  ResamplePolicy(horizon);

  // ----- rollouts (planner.cc:377-415): N perturbed candidates + the nominal as candidate N, one launch
  auto rollouts_start = std::chrono::steady_clock::now();
  int P = resampled_policy.num_spline_points;
  for (int t = 0; t < P; t++) std::copy(resampled_policy.plan.NodeValues(t), resampled_policy.plan.NodeValues(t) + nu_, knot_values_.begin() + (size_t)t * nu_);
  for (int k = 0; k < P * nu_; k++) noise_std_[k] = std::max(std::sqrt(variance[k]), std_min_);   // AddNoiseToPolicy, planner.cc:359-362
  MjpcHipPlanInput in = PlanInput(times_scratch.data(), knot_values_.data(), P, (int)resampled_policy.plan.Interpolation(),
                                  num_trajectory + 1, horizon);
  in.noise_eps = injected_noise_eps; in.seed = seed; in.stream = plan_iter++;
  in.noise_std = noise_std_.data(); in.nominal_index = num_trajectory;
  MjpcHipPlanOutput out;
  std::memset(&out, 0, sizeof(out));
  out.returns = returns.data(); out.failure = failures.data();
  if (mjpc_hip_plan(engine_, &in, &out) != 0) { Fatal(mjpc_hip_last_error()); return; }
  noise_compute_time = out.noise_compute_time_us;
  last_horizon_ = horizon;
  // nominal trajectory = candidate N
  MjpcHipPlanOutput nom = TrajectoryOutput(nominal_trajectory);
  if (mjpc_hip_get_candidate(engine_, num_trajectory, &nom) != 0) { Fatal(mjpc_hip_last_error()); return; }
  nominal_trajectory.horizon = horizon; nominal_trajectory.total_return = returns[num_trajectory];
  nominal_trajectory.failure = failures[num_trajectory] != 0;
  all_knots_.resize((size_t)(num_trajectory + 1) * P * nu_);
  if (mjpc_hip_get_knots(engine_, all_knots_.data()) != 0) { Fatal(mjpc_hip_last_error()); return; }
  OrderCandidates(num_trajectory);
  rollouts_compute_time = Micros(rollouts_start);

  // ----- update policy (planner.cc:205-283)
  auto policy_update_start = std::chrono::steady_clock::now();
  int num_parameters = P * nu_;
  double avg_return = 0.0;
  std::fill(parameters_scratch.begin(), parameters_scratch.end(), 0.0);
  for (int i = 0; i < n_elite; i++) {
    int idx = trajectory_order[i];
    const double* kn = all_knots_.data() + (size_t)idx * num_parameters;
    for (int k = 0; k < num_parameters; k++) parameters_scratch[k] += kn[k];
    avg_return += returns[idx];
  }
  for (int k = 0; k < num_parameters; k++) parameters_scratch[k] *= 1.0 / n_elite;     // mju_scl
  avg_return /= n_elite;
  std::fill(variance.begin(), variance.end(), 0.0);
  {
    const double* best = all_knots_.data() + (size_t)trajectory_order[0] * num_parameters;   // the reference reads elite 0 for every i
    for (int k = 0; k < num_parameters; k++) {
      double p_avg = parameters_scratch[k];
      for (int i = 0; i < n_elite; i++) {
        double diff = best[k] - p_avg;
        variance[k] += diff * diff / (n_elite - 1);
      }
    }
  }
  {
    const std::unique_lock<std::shared_mutex> lock(mtx_);
    policy.plan.Clear();
    policy.plan.SetInterpolation((SplineInterpolation)interpolation_);
    for (int t = 0; t < P; t++) policy.plan.AddNode(times_scratch[t], parameters_scratch.data() + (size_t)t * nu_);
  }
  improvement = std::max(avg_return - returns[trajectory_order[0]], 0.0);
  policy_update_compute_time = Micros(policy_update_start);
}

void CrossEntropyPlanner::NominalTrajectory(int horizon) {   // planner.cc:286-297: rollout of resampled_policy
  RolloutNominal(engine_, resampled_policy.plan, horizon, nominal_trajectory);
}

const Trajectory* CrossEntropyPlanner::BestTrajectory() { return &nominal_trajectory; }

void SamplingPlanner::CandidateKnots(int candidate, double* out) {
  FetchCandidate(trajectory_order[candidate]);
  std::copy(winner_knots_.begin(), winner_knots_.end(), out);
}

// trajectory[i] / candidate_policy[i] of the reference by BATCH index i (not ranked): what iLQS reads (ilqs/planner.cc:98-198)
void SamplingPlanner::FetchCandidateUnranked(int index) { FetchCandidate(index); trajectory_winner.horizon = last_horizon_;
  trajectory_winner.total_return = returns[index]; trajectory_winner.failure = failures[index] != 0; }
void SamplingPlanner::CandidateKnotsUnranked(int index, double* out) {
  FetchCandidate(index);
  std::copy(winner_knots_.begin(), winner_knots_.end(), out);
}
// every candidate's trace rows of the last plan step, [num_trajectory][horizon][3 * num_trace]: SamplingPlanner::Traces
void SamplingPlanner::AllTraces(double* out) {
  if (mjpc_hip_multi_get_traces(engine_, out) != 0) Fatal(mjpc_hip_last_error());
}

void SetErrorHandler(void (*handler)(const char*)) { g_error_handler = handler; }

// ------------------------------------------------------------------ RobustPlanner
RobustPlanner::~RobustPlanner() { if (engine_) mjpc_hip_destroy(engine_); }

void RobustPlanner::Initialize(const MjpcHipModel* model, const MjpcHipTask* task, const Numerics& numerics) {   // robust_planner.cc:30-58
  numerics_ = numerics;
  delegate.Initialize(model, task, numerics);
  nu_ = model->nu;
  nrepetitions_ = numerics.robust_repetitions;
  ncandidates_ = numerics.robust_candidates;
  if (ncandidates_ == -1) ncandidates_ = numerics.sampling_trajectories / nrepetitions_;
  xfrc_std_ = numerics.robust_xfrc; xfrc_rate_ = numerics.robust_xfrc_rate;
  if (engine_) { mjpc_hip_destroy(engine_); engine_ = nullptr; }
  int cap = std::max(1, std::max(ncandidates_, 1) * std::max(nrepetitions_, 1));
  engine_ = mjpc_hip_create(model, task, cap, numerics.max_horizon, numerics.device);
  if (!engine_) Fatal(mjpc_hip_last_error());
}
void RobustPlanner::SetTask(const MjpcHipTask* task) {
  delegate.SetTask(task);
  if (mjpc_hip_set_task(engine_, task) != 0) Fatal(mjpc_hip_last_error());
}

void RobustPlanner::OptimizePolicy(int horizon) {   // robust_planner.cc:91-157
  // Conscious fix of a reference quirk: at this snapshot RobustPlanner calls the delegate's OptimizePolicyCandidates directly
  // (robust_planner.cc:93) and UpdateNominalPolicy only runs inside SamplingPlanner::OptimizePolicy (planner.cc:192), so the
  // wrapped planner never re-times its knots to the current time.  Resample first, as OptimizePolicy does.
  delegate.UpdateNominalPolicy(horizon);
  int ncandidates = delegate.OptimizePolicyCandidates(ncandidates_, horizon);
  best_candidate = -1;
  if (!ncandidates) return;
  if (ncandidates == 1) { delegate.CopyCandidateToPolicy(0); best_candidate = 0; return; }
  int repetitions = nrepetitions_;
  const std::vector<double>& kt = delegate.KnotTimes();
  int P = (int)kt.size();
  size_t row = (size_t)P * nu_;
  cand_knots_.resize((size_t)ncandidates * repetitions * row);
  for (int i = 0; i < ncandidates; i++) {
    delegate.CandidateKnots(i, cand_knots_.data() + (size_t)i * repetitions * row);
    for (int j = 1; j < repetitions; j++)
      std::copy(cand_knots_.begin() + (size_t)i * repetitions * row, cand_knots_.begin() + ((size_t)i * repetitions + 1) * row,
                cand_knots_.begin() + ((size_t)i * repetitions + j) * row);
  }
  int total = ncandidates * repetitions;
  noisy_returns.assign(total, 0.0); noisy_failures.assign(total, 0);
  std::vector<double> zeros(row, 0.0);
  MjpcHipPlanInput in = MakePlanInput(delegate.state.data(), delegate.mocap.data(), delegate.userdata.data(), delegate.time, kt.data(),
                                      zeros.data(), P, delegate.interpolation_, total, horizon);
  in.candidate_knots = cand_knots_.data(); in.xfrc_std = xfrc_std_; in.xfrc_rate = xfrc_rate_;
  in.seed = seed; in.stream = plan_iter++;
  MjpcHipPlanOutput out;
  std::memset(&out, 0, sizeof(out));
  out.returns = noisy_returns.data(); out.failure = noisy_failures.data();
  if (mjpc_hip_plan(engine_, &in, &out) != 0) { Fatal(mjpc_hip_last_error()); return; }
  // mean over the delegate's score and the valid noisy rollouts; the best mean wins (robust_planner.cc:128-151)
  candidate_scores.assign(ncandidates, 0.0);
  double best_score = 0;
  for (int candidate = 0; candidate < ncandidates; candidate++) {
    double mean_return = delegate.CandidateScore(candidate);
    int valid_rollouts = 0;
    for (int j = 0; j < repetitions; j++) {
      if (noisy_failures[repetitions * candidate + j]) continue;
      double total_return = noisy_returns[repetitions * candidate + j];
      mean_return = (valid_rollouts * mean_return + total_return) / (valid_rollouts + 1);
      valid_rollouts++;
    }
    candidate_scores[candidate] = mean_return;
    if (best_candidate == -1 || mean_return < best_score) { best_candidate = candidate; best_score = mean_return; }
  }
  delegate.CopyCandidateToPolicy(best_candidate);
}


// ------------------------------------------------------------------ SampleGradientPlanner
SampleGradientPlanner::~SampleGradientPlanner() { if (engine_) mjpc_hip_destroy(engine_); }

void SampleGradientPlanner::Initialize(const MjpcHipModel* model, const MjpcHipTask* task, const Numerics& numerics) {   // planner.cc:43-75
  noise_exploration = numerics.sampling_exploration[0];
  num_gradient_ = numerics.sample_gradient_trajectories;
  gradient_filter_ = numerics.sample_gradient_filter;
  if (!InitializeCommon(model, task, numerics)) return;
  if (engine_) { mjpc_hip_destroy(engine_); engine_ = nullptr; }
  engine_ = mjpc_hip_create(model, task, numerics.max_samples, numerics.max_horizon, numerics.device);
  if (!engine_) { Fatal(mjpc_hip_last_error()); return; }
  policy.Allocate(model, numerics.sampling_spline_points);
  resampled_policy.Allocate(model, numerics.sampling_spline_points);
  previous_policy.Allocate(model, numerics.sampling_spline_points);
}

void SampleGradientPlanner::Allocate() {   // planner.cc:78-118
  AllocateState();
  plan_scratch_ = TimeSpline(nu_);
  trajectory_order.resize(numerics_.max_samples);
  std::iota(trajectory_order.begin(), trajectory_order.end(), 0);
  returns.assign(numerics_.max_samples, 0.0); failures.assign(numerics_.max_samples, 0);
  candidate_policy_.resize(numerics_.max_samples);
  for (auto& c : candidate_policy_) { c.nu = nu_; c.ctrlrange = ctrlrange_; c.num_spline_points = policy.num_spline_points; c.plan = TimeSpline(nu_); }
  candidate_valid_.assign(numerics_.max_samples, 1);
  SizeTrajectory(trajectory_winner);
  int num_max_parameter = nu_ * MaxSamplingSplinePoints;       // the engine's spline capacity
  gradient.assign(num_max_parameter, 0.0); gradient_previous.assign(num_max_parameter, 0.0);
}

void SampleGradientPlanner::Reset(int horizon, const double* initial_repeated_action) {   // planner.cc:121-160
  ResetState(horizon, initial_repeated_action);
  resampled_policy.Reset(horizon, initial_repeated_action);
  plan_scratch_.Clear();
  if (engine_ && mjpc_hip_noise_history_reset(engine_) != 0) Fatal(mjpc_hip_last_error());      // std::fill(noise, 0)
  for (size_t i = 0; i < candidate_policy_.size(); i++) { candidate_policy_[i].Reset(horizon); candidate_valid_[i] = 1; }
  improvement = 0.0;
  winner = 0;
  std::fill(gradient.begin(), gradient.end(), 0.0);
  std::fill(gradient_previous.begin(), gradient_previous.end(), 0.0);
}

void SampleGradientPlanner::SetTask(const MjpcHipTask* task) {
  if (mjpc_hip_set_task(engine_, task) != 0) Fatal(mjpc_hip_last_error());
}

void SampleGradientPlanner::ResamplePolicy(SamplingPolicy& p, int horizon, int num_spline_points) {   // planner.cc:302-326
  double nominal_time = time;
  double time_shift = std::max((horizon - 1) * timestep_ / (num_spline_points - 1), 1.0e-5);
  plan_scratch_.Clear();
  plan_scratch_.SetInterpolation(p.plan.Interpolation());
  for (int t = 0; t < num_spline_points; t++) {
    double* node = plan_scratch_.AddNode(nominal_time);
    p.Action(node, nullptr, nominal_time);
    nominal_time += time_shift;
  }
  p.plan = plan_scratch_;
  p.num_spline_points = num_spline_points;
}

// candidate_policy[index] of the reference.  Only explicit candidates are kept as splines; a noisy candidate of the last plan is
// rebuilt from its rolled-out knots when somebody asks for it (the sliders moved and its slot became a gradient slot).
SamplingPolicy& SampleGradientPlanner::Candidate(int index) {
  SamplingPolicy& c = candidate_policy_[index];
  if (!candidate_valid_[index]) {
    c.plan = TimeSpline(nu_, (SplineInterpolation)last_interp_);
    if (index < last_N_)
      for (int t = 0; t < last_P_; t++) c.plan.AddNode(knot_times_[t], all_knots_.data() + ((size_t)index * last_P_ + t) * nu_);
    c.num_spline_points = last_P_;
    candidate_valid_[index] = 1;
  }
  return c;
}

int SampleGradientPlanner::CandidatePolicy(int index, double* times, double* values) {
  return CopyKnots(Candidate(index), times, values);
}

void SampleGradientPlanner::OptimizePolicy(int horizon) {   // planner.cc:169-273
  int num_trajectory = num_trajectory_;
  num_gradient_ = std::min(num_gradient_, num_trajectory - 1);
  int num_gradient = num_gradient_;
  int num_noisy = num_trajectory - num_gradient;
  int num_spline_points = policy.num_spline_points;
  if (num_spline_points < 1 || num_spline_points > MaxSamplingSplinePoints) { Fatal("SampleGradientPlanner: spline points out of range (1..36)"); return; }
  policy.plan.SetInterpolation((SplineInterpolation)interpolation_);
  {
    const std::shared_lock<std::shared_mutex> lock(mtx_);
    resampled_policy.CopyFrom(policy, num_spline_points);
  }
  resampled_policy.num_spline_points = num_spline_points;
  ResamplePolicy(resampled_policy, horizon, num_spline_points);
  for (int i = 0; i < num_gradient; i++) ResamplePolicy(Candidate(num_noisy + i), horizon, num_spline_points);

  // ----- rollouts (planner.cc:358-398): nominal, noisy and gradient candidates in one launch
  auto rollouts_start = std::chrono::steady_clock::now();
  int P = num_spline_points;
  size_t row = (size_t)P * nu_;
  KnotArrays(resampled_policy.plan, knot_times_, knot_values_);       // P nodes: ResamplePolicy has just laid them
  noise_std_.assign(row, noise_exploration);
  cand_table_.resize((size_t)num_trajectory * row);             // rows below num_noisy are not read by the engine
  for (int i = num_noisy; i < num_trajectory; i++) {
    const SamplingPolicy& c = candidate_policy_[i];
    for (int t = 0; t < P; t++) std::copy(c.plan.NodeValues(t), c.plan.NodeValues(t) + nu_, cand_table_.begin() + (size_t)i * row + (size_t)t * nu_);
  }
  MjpcHipPlanInput in = PlanInput(knot_times_.data(), knot_values_.data(), P, (int)resampled_policy.plan.Interpolation(),
                                  num_trajectory, horizon);
  in.noise_eps = injected_noise_eps; in.seed = seed; in.stream = plan_iter++;
  in.noise_std = noise_std_.data(); in.nominal_index = 0;
  in.candidate_knots = cand_table_.data();
  MjpcHipPlanOutput out;
  std::memset(&out, 0, sizeof(out));
  out.returns = returns.data(); out.failure = failures.data();
  if (mjpc_hip_plan_mixed(engine_, &in, num_noisy, &out) != 0) { Fatal(mjpc_hip_last_error()); return; }
  noise_compute_time = out.noise_compute_time_us;
  all_knots_.resize((size_t)num_trajectory * row);
  if (mjpc_hip_get_knots(engine_, all_knots_.data()) != 0) { Fatal(mjpc_hip_last_error()); return; }
  last_horizon_ = horizon; last_N_ = num_trajectory; last_P_ = P; last_interp_ = in.interpolation;
  for (int i = 0; i < num_noisy; i++) candidate_valid_[i] = 0;        // candidate_policy[i] = row i of all_knots_ now
  rollouts_compute_time = Micros(rollouts_start);

  // ----- update policy (planner.cc:216-262)
  auto policy_update_start = std::chrono::steady_clock::now();
  OrderCandidates(num_trajectory);
  const int idx_nominal = 0;
  if (returns[trajectory_order[0]] < returns[idx_nominal]) winner = trajectory_order[0];
  else winner = idx_nominal;
  if (winner > idx_nominal) winner_type_ = winner < num_trajectory - num_gradient ? kPerturb : kGradient;
  else winner_type_ = kNominal;
  {
    const SamplingPolicy& w = Candidate(winner);
    const std::unique_lock<std::shared_mutex> lock(mtx_);
    policy.plan = w.plan;
  }
  improvement = std::max(returns[idx_nominal] - returns[winner], 0.0);
  {
    MjpcHipPlanOutput best = TrajectoryOutput(trajectory_winner);
    if (mjpc_hip_get_candidate(engine_, winner, &best) != 0) { Fatal(mjpc_hip_last_error()); return; }
    trajectory_winner.horizon = horizon; trajectory_winner.total_return = returns[winner]; trajectory_winner.failure = failures[winner] != 0;
  }
  policy_update_compute_time = Micros(policy_update_start);

  // ----- gradient candidates for the next plan step (planner.cc:264-272)
  auto gradient_start = std::chrono::steady_clock::now();
  GradientCandidates(num_trajectory, num_gradient, horizon);
  gradient_candidates_compute_time = Micros(gradient_start);
}

void SampleGradientPlanner::ReturnWeights(const int* order, int num_noisy, double* weights) {   // planner.cc:437-449
  double f0 = std::log(0.5 * num_noisy + 1.0);
  double den = 0.0;
  for (int i = 0; i < num_noisy; i++) den += std::max(0.0, f0 - std::log(order[i] + 1));
  for (int i = 0; i < num_noisy; i++) weights[i] = std::max(0.0, f0 - std::log(order[i] + 1)) / den - 1.0 / num_noisy;
}

void SampleGradientPlanner::LogScale(double* values, double max_value, double min_value, int steps) {   // utilities.cc:802-808
  double step = (std::log(max_value) - std::log(min_value)) / std::max((steps - 1), 1);
  for (int i = 0; i < steps; i++) values[i] = std::exp(std::log(min_value) + i * step);
  // the scale starts at min_value itself: exp(log(1e-3)) comes out one ulp above 1e-3 with glibc, and the smallest step is a
  // documented constant of the planner (gradient_min_step_size), not a libm artefact
  if (steps > 0) values[0] = min_value;
}

void SampleGradientPlanner::GradientCandidates(int num_trajectory, int num_gradient, int) {   // planner.cc:401-493
  if (num_gradient < 1) return;
  int num_spline_points = resampled_policy.num_spline_points;
  int num_parameters = num_spline_points * nu_;
  std::copy(gradient.begin(), gradient.begin() + num_parameters, gradient_previous.begin());
  int num_noisy = num_trajectory - num_gradient;
  // fitness shaping, computed when the count of noisy candidates changes and only then (planner.cc:419-450)
  if ((int)return_weight_.size() != num_noisy) {
    return_weight_.resize(num_noisy);
    OrderCandidates(num_noisy);
    ReturnWeights(trajectory_order.data(), num_noisy, return_weight_.data());
  }
  // gradient = sum_i noise[trajectory_order[i]] * return_weight_[i] / num_noisy, on the device over the noise history
  scale_.resize(num_noisy);
  for (int i = 0; i < num_noisy; i++) scale_[i] = return_weight_[i] / num_noisy;
  std::fill(gradient.begin(), gradient.end(), 0.0);
  if (mjpc_hip_sample_gradient(engine_, num_noisy, trajectory_order.data(), scale_.data(), gradient.data()) != 0) { Fatal(mjpc_hip_last_error()); return; }
  if ((int)step_size_.size() != num_gradient) {
    step_size_.resize(num_gradient);
    LogScale(step_size_.data(), gradient_max_step_size, gradient_min_step_size, num_gradient);
  }
  double gradient_filter = gradient_filter_;
  for (int i = num_noisy; i < num_trajectory; i++) {
    SamplingPolicy& c = candidate_policy_[i];
    c.CopyFrom(resampled_policy, num_spline_points);
    candidate_valid_[i] = 1;
    double scaling = step_size_[i - num_noisy] / noise_exploration;
    for (int t = 0; t < (int)c.plan.Size(); t++) {
      double* n = c.plan.NodeValues(t);
      for (int k = 0; k < nu_; k++) n[k] += gradient[(size_t)t * nu_ + k] * (-scaling * gradient_filter);                     // mju_addToScl
      for (int k = 0; k < nu_; k++) n[k] += gradient_previous[(size_t)t * nu_ + k] * (-scaling * (1.0 - gradient_filter));
      for (int k = 0; k < nu_; k++) n[k] = std::max(ctrlrange_[2 * k], std::min(ctrlrange_[2 * k + 1], n[k]));                  // Clamp
    }
  }
}

void SampleGradientPlanner::NominalTrajectory(int horizon) {   // planner.cc:276-287: rollout of resampled_policy into trajectory[0]
  if (!RolloutNominal(engine_, resampled_policy.plan, horizon, trajectory_winner, &failures[0])) return;
  returns[0] = trajectory_winner.total_return;
  winner = 0;                                          // BestTrajectory() shows trajectory[0] until the next OptimizePolicy
}

const Trajectory* SampleGradientPlanner::BestTrajectory() { return &trajectory_winner; }

// ------------------------------------------------------------------ ModelDerivatives
void ModelDerivatives::Allocate(int nd, int nu, int nr, int T, int ds) {
  dim_state_derivative = nd; dim_action = nu; dim_sensor = nr;
  if (ds > 0) dim_state = ds;
  A.resize((size_t)T * nd * nd); B.resize((size_t)T * nd * nu); C.resize((size_t)T * nr * nd); D.resize((size_t)T * nr * nu);
  failure.resize(T);
}

void ModelDerivatives::Reset(int nd, int nu, int nr, int T) {
  if (nd != dim_state_derivative || nu != dim_action || nr != dim_sensor || (size_t)T > failure.size()) Allocate(nd, nu, nr, T);
  std::fill(A.begin(), A.begin() + (size_t)T * nd * nd, 0.0);
  std::fill(B.begin(), B.begin() + (size_t)T * nd * nu, 0.0);
  std::fill(C.begin(), C.begin() + (size_t)T * nr * nd, 0.0);
  std::fill(D.begin(), D.begin() + (size_t)T * nr * nu, 0.0);
  std::fill(failure.begin(), failure.begin() + T, 0);
}

// model_derivatives.cc:56-72.  The reference pushes 0, then s, 2s, ... below T - s, then T - 2 and T - 1, which names an index
// twice when T is small (T = 2: 0, 0, 1); its interpolate_ walk then still skips exactly the indices named at least once.  Here
// the list is that set, ascending.
void ModelDerivatives::IndexSets(int T, int skip) {
  evaluate_.clear(); interpolate_.clear();
  if (T < 2) { Fatal("ModelDerivatives: T < 2"); return; }
  const int s = (skip < 0 ? 0 : skip) + 1;
  evaluate_.push_back(0);
  for (int t = s; t < T - s; t += s) evaluate_.push_back(t);
  if (T - 2 > evaluate_.back()) evaluate_.push_back(T - 2);
  evaluate_.push_back(T - 1);
  for (int t = 0, e = 0; t < T; t++) {
    if (e == (int)evaluate_.size() || evaluate_[e] > t) interpolate_.push_back(t);
    else e++;
  }
}

// model_derivatives.cc:108-161: FindInterval (utilities.h:122-141) over evaluate_, tt = (t - e0) / (e1 - e0), then mju_scl by
// 1 - tt and mju_addToScl by tt (two rounded products and one rounded sum per entry; this file is compiled without contraction)
void ModelDerivatives::Interpolate() {
  const size_t n[4] = {(size_t)dim_state_derivative * dim_state_derivative, (size_t)dim_state_derivative * dim_action,
                       (size_t)dim_sensor * dim_state_derivative, (size_t)dim_sensor * dim_action};
  std::vector<double>* blk[4] = {&A, &B, &C, &D};
  for (int t : interpolate_) {
    int ub = (int)(std::upper_bound(evaluate_.begin(), evaluate_.end(), t) - evaluate_.begin());
    int b0 = ub - 1, b1 = ub;
    if (b0 < 0) { b0 = 0; b1 = 0; }
    else if (b1 > (int)evaluate_.size() - 1) b1 = (int)evaluate_.size() - 1;
    const int e0 = evaluate_[b0], e1 = evaluate_[b1];
    double tt = (b0 == b1) ? 0.0 : double(t - e0) / double(e1 - e0);
    for (int k = 0; k < 4; k++) {
      double* out = blk[k]->data() + (size_t)t * n[k];
      const double *L = blk[k]->data() + (size_t)e0 * n[k], *U = blk[k]->data() + (size_t)e1 * n[k];
      for (size_t i = 0; i < n[k]; i++) out[i] = L[i] * (1.0 - tt);
      for (size_t i = 0; i < n[k]; i++) out[i] += U[i] * tt;
    }
  }
}

bool ModelDerivatives::Compute(MjpcHipEngine* engine, const double* x, const double* u, const double* h, int T, double tol, int mode, int skip,
                               const double* mocap, const double* userdata) {
  if (T < 2) { Fatal("ModelDerivatives: T < 2"); return false; }
  const int nd = dim_state_derivative, nu = dim_action, nr = dim_sensor;
  if ((size_t)T > failure.size()) Allocate(nd, nu, nr, T);
  IndexSets(T, skip);
  // rows of the evaluated knots, gathered: one device call
  const size_t ne = evaluate_.size();
  const int ds = dim_state;
  if (ds < 1) { Fatal("ModelDerivatives: dim_state is not set (Allocate's last argument: nq + nv + na)"); return false; }
  gx_.resize(ne * ds); gu_.resize(ne * nu + 1); gh_.resize(ne);
  gA_.resize(ne * nd * nd); gB_.resize(ne * nd * nu + 1); gC_.resize(ne * nr * nd + 1); gD_.resize(ne * nr * nu + 1); gfail_.resize(ne);
  for (size_t k = 0; k < ne; k++) {
    const int t = evaluate_[k];
    std::copy(x + (size_t)t * ds, x + (size_t)(t + 1) * ds, gx_.begin() + k * ds);
    std::copy(u + (size_t)t * nu, u + (size_t)(t + 1) * nu, gu_.begin() + k * nu);
    gh_[k] = h[t];
  }
  if (mjpc_hip_transition_fd(engine, (int)ne, gx_.data(), gu_.data(), gh_.data(), mocap, userdata, tol, mode, 1, gA_.data(), gB_.data(), gC_.data(),
                             gD_.data(), gfail_.data()) != 0) return false;
  std::fill(failure.begin(), failure.begin() + T, 0);
  for (size_t k = 0; k < ne; k++) {
    const size_t t = (size_t)evaluate_[k];
    failure[t] = gfail_[k];
    std::copy(gC_.begin() + k * nr * nd, gC_.begin() + (k + 1) * nr * nd, C.begin() + t * nr * nd);
    if ((int)t == T - 1) continue;                    // terminal knot: C only
    std::copy(gA_.begin() + k * nd * nd, gA_.begin() + (k + 1) * nd * nd, A.begin() + t * nd * nd);
    std::copy(gB_.begin() + k * nd * nu, gB_.begin() + (k + 1) * nd * nu, B.begin() + t * nd * nu);
    std::copy(gD_.begin() + k * nr * nu, gD_.begin() + (k + 1) * nr * nu, D.begin() + t * nr * nu);
  }
  Interpolate();
  return true;
}

// ------------------------------------------------------------------ InverseDerivatives
void InverseDerivatives::Allocate(int ds, int nq, int nv, int nu, int nr, int T) {
  dim_state = ds; dim_q = nq; dim_v = nv; dim_action = nu; dim_sensor = nr;
  for (std::vector<double>* b : {&DfDq, &DfDv, &DfDa}) b->resize((size_t)T * nv * nv);
  for (std::vector<double>* b : {&DsDq, &DsDv, &DsDa}) b->resize((size_t)T * nr * nv);
  failure.resize(T);
  row_stage.assign(nr, kStageAcc);
}

void InverseDerivatives::Reset(int T) {
  if ((size_t)T > failure.size()) { std::vector<int> keep = row_stage; Allocate(dim_state, dim_q, dim_v, dim_action, dim_sensor, T); row_stage = keep; }
  const size_t nv = dim_v, nr = dim_sensor;
  for (std::vector<double>* b : {&DfDq, &DfDv, &DfDa}) std::fill(b->begin(), b->begin() + (size_t)T * nv * nv, 0.0);
  for (std::vector<double>* b : {&DsDq, &DsDv, &DsDa}) std::fill(b->begin(), b->begin() + (size_t)T * nr * nv, 0.0);
  std::fill(failure.begin(), failure.begin() + T, 0);
}

void InverseDerivatives::SetRowStages(const int* stage) { row_stage.assign(stage, stage + dim_sensor); }

bool InverseDerivatives::RowStagesFromTable(const MjpcHipTask* task, int* stage) {
  if (!task || task->task_id != MJPC_TASK_TABLE || task->num_int < 3 || !task->int_data) return false;
  const int* d = task->int_data;
  const int nblock = d[1], nterm = d[2];
  if (nblock < 0 || nterm < 0 || task->num_int < 3 + 6 * nblock + 4 * nterm) return false;
  const int *B = d + 3, *Tm = B + 6 * nblock;
  for (int i = 0; i < task->num_residual; i++) stage[i] = kStagePos;
  for (int b = 0; b < nblock; b++, B += 6) {
    int st = kStagePos;
    for (int j = B[4]; j < B[4] + B[5] && j < nterm; j++) {
      const int kind = Tm[4 * j];
      const int ks = (kind >= MJPC_TBL_QACC || kind == MJPC_TBL_ACTUATOR_FORCE) ? kStageAcc
                     : (kind == MJPC_TBL_QVEL || kind == MJPC_TBL_SUBTREE_LINVEL || kind == MJPC_TBL_LINVEL || kind == MJPC_TBL_ANGVEL) ? kStageVel : kStagePos;
      if (ks > st) st = ks;
    }
    for (int i = B[1]; i < B[1] + B[2] && i < task->num_residual; i++) if (i >= 0) stage[i] = st;
  }
  return true;
}

bool InverseDerivatives::Compute(MjpcHipEngine* engine, const double* x, const double* u, const double* a, const double* h, int T, double tol, int mode,
                                 int discrete, const double* mocap, const double* userdata) {
  if (T < 1) { Fatal("InverseDerivatives: T < 1"); return false; }
  if (dim_state < 1) { Fatal("InverseDerivatives: not allocated"); return false; }
  const size_t ds = dim_state, nq = dim_q, nv = dim_v, nr = dim_sensor;
  Reset(T);
  // the window's rows with the ends as the reference evaluates them: zero velocity and acceleration at 0, zero acceleration at T - 1
  gx_.assign(x, x + (size_t)T * ds); ga_.assign(a, a + (size_t)T * nv);
  std::fill(gx_.begin() + nq, gx_.begin() + nq + nv, 0.0);
  std::fill(ga_.begin(), ga_.begin() + nv, 0.0);
  std::fill(ga_.begin() + (size_t)(T - 1) * nv, ga_.begin() + (size_t)T * nv, 0.0);
  if (mjpc_hip_inverse_fd(engine, T, gx_.data(), u, ga_.data(), h, mocap, userdata, discrete, tol, mode, DfDq.data(), DfDv.data(), DfDa.data(),
                          nr ? DsDq.data() : nullptr, nr ? DsDv.data() : nullptr, nr ? DsDa.data() : nullptr, failure.data()) != 0) return false;
  auto zero_block = [&](std::vector<double>& b, size_t t, size_t rows) { std::fill(b.begin() + t * rows * nv, b.begin() + (t + 1) * rows * nv, 0.0); };
  auto zero_rows = [&](std::vector<double>& b, size_t t, int from_stage) {
    for (size_t i = 0; i < nr; i++) if (row_stage[i] >= from_stage) std::fill(b.begin() + (t * nr + i) * nv, b.begin() + (t * nr + i + 1) * nv, 0.0);
  };
  // the last configuration first: a window of one configuration is a first one
  if (T > 1) {
    const size_t t = (size_t)T - 1;
    zero_block(DfDq, t, nv); zero_block(DfDv, t, nv); zero_block(DfDa, t, nv); zero_block(DsDa, t, nr);
    zero_rows(DsDq, t, kStageAcc); zero_rows(DsDv, t, kStageAcc);
  }
  zero_block(DfDq, 0, nv); zero_block(DfDv, 0, nv); zero_block(DfDa, 0, nv); zero_block(DsDv, 0, nr); zero_block(DsDa, 0, nr);
  zero_rows(DsDq, 0, kStageVel);
  return true;
}

// ------------------------------------------------------------------ CostDerivatives
void CostDerivatives::Allocate(int nd, int nu, int nr, int T) {
  dim_state_derivative = nd; dim_action = nu; dim_residual = nr; horizon = T;
  cr.resize((size_t)T * nr); cx.resize((size_t)T * nd); cu.resize((size_t)T * nu);
  cxx.resize((size_t)T * nd * nd); cuu.resize((size_t)T * nu * nu); cxu.resize((size_t)T * nd * nu);
}

void CostDerivatives::Reset(int nd, int nu, int nr, int T) {
  if (nd != dim_state_derivative || nu != dim_action || nr != dim_residual || T > horizon) Allocate(nd, nu, nr, T);
  for (std::vector<double>* v : {&cr, &cx, &cu, &cxx, &cuu, &cxu}) std::fill(v->begin(), v->end(), 0.0);
}

bool CostDerivatives::Compute(MjpcHipEngine* engine, const double* r, const double* rx, const double* ru, int nd, int nu, int nr, int T, bool hessians) {
  Reset(nd, nu, nr, T);
  return mjpc_hip_cost_derivatives(engine, T, r, rx, ru, 1, hessians ? 1 : 0, cr.data(), cx.data(), cu.data(), cxx.data(), cuu.data(), cxu.data()) == 0;
}

// ------------------------------------------------------------------ Gradient
void Gradient::Allocate(int nd, int nu, int T) {
  Vx.resize((size_t)nd * T); Qx.resize((size_t)nd * (T > 1 ? T - 1 : 0)); Qu.resize((size_t)nu * (T > 1 ? T - 1 : 0));
}

void Gradient::Reset(int nd, int nu, int T) {
  if (Vx.size() < (size_t)nd * T || Qx.size() + nd < (size_t)nd * T || Qu.size() + nu < (size_t)nu * T) Allocate(nd, nu, T);
  std::fill(Vx.begin(), Vx.end(), 0.0); std::fill(Qx.begin(), Qx.end(), 0.0); std::fill(Qu.begin(), Qu.end(), 0.0);
  dV[0] = 0.0; dV[1] = 0.0;
}

int Gradient::Compute(double* k, const ModelDerivatives* md, const CostDerivatives* cd, int nd, int nu, int T) {
  return Compute(k, md->A.data(), md->B.data(), cd->cx.data(), cd->cu.data(), nd, nu, T);
}

// gradient.cc:43-108.  Every contraction starts at 0.0 and runs over the ascending row of A / B, a rounded product and a rounded add
// per step (this file is compiled without contraction): the device's gd_column / gd_dv (csrc/cost_derivatives.h) bit for bit.
// GradientStep cannot fail, so the reference's early exit is not restated and the status is always 0.
int Gradient::Compute(double* k, const double* A, const double* B, const double* cx, const double* cu, int nd, int nu, int T) {
  if (T < 2) { Fatal("Gradient: T < 2"); return -1; }
  if (Vx.size() < (size_t)nd * T || Qx.size() < (size_t)nd * (T - 1) || Qu.size() < (size_t)nu * (T - 1)) Allocate(nd, nu, T);
  dV[0] = 0.0; dV[1] = 0.0;
  std::copy(cx + (size_t)(T - 1) * nd, cx + (size_t)T * nd, Vx.begin() + (size_t)(T - 1) * nd);
  for (int t = T - 1; t > 0; t--) {
    const double *Wx = Vx.data() + (size_t)t * nd, *At = A + (size_t)(t - 1) * nd * nd, *Bt = B + (size_t)(t - 1) * nd * nu;
    double *Qxt = Qx.data() + (size_t)(t - 1) * nd, *Qut = Qu.data() + (size_t)(t - 1) * nu, *kt = k + (size_t)(t - 1) * nu;
    for (int c = 0; c < nd; c++) {
      double q = 0.0;
      for (int r = 0; r < nd; r++) q += At[(size_t)r * nd + c] * Wx[r];
      Qxt[c] = q + cx[(size_t)(t - 1) * nd + c];
    }
    for (int c = 0; c < nu; c++) {
      double q = 0.0;
      for (int r = 0; r < nd; r++) q += Bt[(size_t)r * nu + c] * Wx[r];
      Qut[c] = q + cu[(size_t)(t - 1) * nu + c];
    }
    double d = 0.0;
    for (int c = 0; c < nu; c++) { kt[c] = -Qut[c]; d += kt[c] * Qut[c]; }
    std::copy(Qxt, Qxt + nd, Vx.begin() + (size_t)(t - 1) * nd);
    dV[0] += d;
  }
  std::copy(k + (size_t)(T - 2) * nu, k + (size_t)(T - 1) * nu, k + (size_t)(T - 1) * nu);
  return 0;
}

// ------------------------------------------------------------------ interpolation helpers (utilities.h:122-141, utilities.cc:286-404)
void FindInterval(int* bounds, const std::vector<double>& sequence, double value, int length) {
  auto it = std::upper_bound(sequence.begin(), sequence.begin() + length, value);
  int upper_bound = (int)(it - sequence.begin()), lower_bound = upper_bound - 1;
  if (lower_bound < 0) { bounds[0] = 0; bounds[1] = 0; }
  else if (lower_bound > length - 1) { bounds[0] = length - 1; bounds[1] = length - 1; }
  else { bounds[0] = std::max(lower_bound, 0); bounds[1] = std::min(upper_bound, length - 1); }
}
void ZeroInterpolation(double* output, double x, const std::vector<double>& xs, const double* ys, int dim, int length) {
  int bounds[2];
  FindInterval(bounds, xs, x, length);
  std::copy(ys + dim * bounds[0], ys + dim * (bounds[0] + 1), output);
}
void LinearInterpolation(double* output, double x, const std::vector<double>& xs, const double* ys, int dim, int length) {
  int bounds[2];
  FindInterval(bounds, xs, x, length);
  if (bounds[0] == bounds[1]) { std::copy(ys + dim * bounds[0], ys + dim * (bounds[0] + 1), output); return; }
  double t = (x - xs[bounds[0]]) / (xs[bounds[1]] - xs[bounds[0]]);
  for (int i = 0; i < dim; i++) output[i] = ys[dim * bounds[0] + i] * (1.0 - t);       // mju_scl, then mju_addScl
  for (int i = 0; i < dim; i++) output[i] = output[i] + ys[dim * bounds[1] + i] * t;
}
static void CubicCoefficients(double* c, double x, const std::vector<double>& xs, int T) {
  int bounds[2];
  FindInterval(bounds, xs, x, T);
  if (bounds[0] == bounds[1]) { c[0] = 1.0; c[1] = 0.0; c[2] = 0.0; c[3] = 0.0; return; }
  double dx = xs[bounds[1]] - xs[bounds[0]], t = (x - xs[bounds[0]]) / dx;
  c[0] = 2.0 * t * t * t - 3.0 * t * t + 1.0;
  c[1] = (t * t * t - 2.0 * t * t + t) * dx;
  c[2] = -2.0 * t * t * t + 3 * t * t;
  c[3] = (t * t * t - t * t) * dx;
}
static double FiniteDifferenceSlope(double x, const std::vector<double>& xs, const double* ys, int dim, int length, int i) {
  int b[2];
  FindInterval(b, xs, x, length);
  if (b[0] == 0 && b[1] == 0) return length > 2 ? (ys[dim * (b[1] + 1) + i] - ys[dim * b[1] + i]) / (xs[b[1] + 1] - xs[b[1]]) : 0.0;
  if (b[0] == length - 1 && b[1] == length - 1) return length > 2 ? (ys[dim * b[0] + i] - ys[dim * (b[0] - 1) + i]) / (xs[b[0]] - xs[b[0] - 1]) : 0.0;
  if (b[0] == 0) return (ys[dim * b[1] + i] - ys[dim * b[0] + i]) / (xs[b[1]] - xs[b[0]]);
  return 0.5 * (ys[dim * b[1] + i] - ys[dim * b[0] + i]) / (xs[b[1]] - xs[b[0]]) +
         0.5 * (ys[dim * b[0] + i] - ys[dim * (b[0] - 1) + i]) / (xs[b[0]] - xs[b[0] - 1]);
}
void CubicInterpolation(double* output, double x, const std::vector<double>& xs, const double* ys, int dim, int length) {
  int bounds[2];
  FindInterval(bounds, xs, x, length);
  if (bounds[0] == bounds[1]) { std::copy(ys + dim * bounds[0], ys + dim * (bounds[0] + 1), output); return; }
  double c[4];
  CubicCoefficients(c, x, xs, length);
  for (int i = 0; i < dim; i++) {
    double p0 = ys[bounds[0] * dim + i], p1 = ys[bounds[1] * dim + i];
    double m0 = FiniteDifferenceSlope(xs[bounds[0]], xs, ys, dim, length, i), m1 = FiniteDifferenceSlope(xs[bounds[1]], xs, ys, dim, length, i);
    output[i] = c[0] * p0 + c[1] * m0 + c[2] * p1 + c[3] * m1;
  }
}

// ------------------------------------------------------------------ GradientPolicy (gradient/policy.cc)
void GradientPolicy::Allocate(const MjpcHipModel* model, const Numerics& numerics, int horizon) {
  nu = model->nu;
  ctrlrange.assign(model->actuator_ctrlrange, model->actuator_ctrlrange + 2 * nu);
  k.assign((size_t)nu * horizon, 0.0);
  parameters.assign((size_t)nu * horizon, 0.0); parameter_update.assign((size_t)nu * horizon, 0.0); times.assign(horizon, 0.0);
  num_spline_points = numerics.gradient_spline_points;
  num_parameters = nu * num_spline_points;
  representation = numerics.gradient_representation;
}
void GradientPolicy::Reset(int horizon, const double* initial_repeated_action) {
  const size_t n = std::min((size_t)nu * horizon, parameters.size());
  std::fill(k.begin(), k.begin() + n, 0.0);
  for (size_t i = 0; i < n; i++) parameters[i] = initial_repeated_action ? initial_repeated_action[i % nu] : 0.0;
  std::fill(parameter_update.begin(), parameter_update.begin() + n, 0.0);
  std::fill(times.begin(), times.begin() + std::min((size_t)horizon, times.size()), 0.0);
}
void GradientPolicy::Action(double* action, const double*, double time) const {
  int bounds[2];
  FindInterval(bounds, times, time, num_spline_points);
  if (bounds[0] == bounds[1] || representation == kZeroSpline) ZeroInterpolation(action, time, times, parameters.data(), nu, num_spline_points);
  else if (representation == kLinearSpline) LinearInterpolation(action, time, times, parameters.data(), nu, num_spline_points);
  else if (representation == kCubicSpline) CubicInterpolation(action, time, times, parameters.data(), nu, num_spline_points);
  for (int i = 0; i < nu; i++) action[i] = std::max(ctrlrange[2 * i], std::min(ctrlrange[2 * i + 1], action[i]));
}
void GradientPolicy::CopyFrom(const GradientPolicy& p, int horizon) {
  std::copy(p.k.begin(), p.k.begin() + std::min((size_t)horizon * nu, p.k.size()), k.begin());
  std::copy(p.parameters.begin(), p.parameters.begin() + p.num_parameters, parameters.begin());
  std::copy(p.parameter_update.begin(), p.parameter_update.begin() + p.num_parameters, parameter_update.begin());
  std::copy(p.times.begin(), p.times.begin() + p.num_spline_points, times.begin());
  num_spline_points = p.num_spline_points; num_parameters = p.num_parameters; representation = p.representation;
}
void GradientPolicy::CopyParametersFrom(const std::vector<double>& src_parameters, const std::vector<double>& src_times) {
  std::copy(src_parameters.begin(), src_parameters.begin() + (size_t)num_spline_points * nu, parameters.begin());
  std::copy(src_times.begin(), src_times.begin() + num_spline_points, times.begin());
}

// ------------------------------------------------------------------ BoxQP, iLQGPolicy, iLQGBackwardPass (mjpc/planners/ilqg/)
// Host restatement of csrc/riccati.h by its summation rule (this file is compiled without contraction): ascending contraction index
// from 0.0, a rounded product and a rounded add per step, `/` and sqrt correctly rounded.
namespace {
// res [c1][c2] = A' B, A [r1][c1], B [r1][c2]
void MulMatTMat(double* res, const double* A, const double* B, int r1, int c1, int c2) {
  for (int i = 0; i < c1; i++)
    for (int j = 0; j < c2; j++) {
      double s = 0.0;
      for (int k = 0; k < r1; k++) s += A[(size_t)k * c1 + i] * B[(size_t)k * c2 + j];
      res[(size_t)i * c2 + j] = s;
    }
}
// res [r1][c2] = A B, A [r1][c1], B [c1][c2]
void MulMatMat(double* res, const double* A, const double* B, int r1, int c1, int c2) {
  for (int i = 0; i < r1; i++)
    for (int j = 0; j < c2; j++) {
      double s = 0.0;
      for (int k = 0; k < c1; k++) s += A[(size_t)i * c1 + k] * B[(size_t)k * c2 + j];
      res[(size_t)i * c2 + j] = s;
    }
}
// Cholesky of H[index][index] (leading dimension ldh) into R [nf][nf], lower triangle, zeros above; false: a pivot is not > 0
bool CholFactorSub(double* R, const double* H, int ldh, const int* index, int nf) {
  for (int j = 0; j < nf; j++) {
    double s = 0.0;
    for (int k = 0; k < j; k++) s += R[j * nf + k] * R[j * nf + k];
    const double d = H[index[j] * ldh + index[j]] + -s;
    if (!(d > 0)) return false;
    const double l = std::sqrt(d);
    R[j * nf + j] = l;
    for (int i = j + 1; i < nf; i++) {
      double q = 0.0;
      for (int k = 0; k < j; k++) q += R[i * nf + k] * R[j * nf + k];
      R[i * nf + j] = (H[index[i] * ldh + index[j]] + -q) / l;
      R[j * nf + i] = 0.0;
    }
  }
  return true;
}
void CholSolveSub(double* x, const double* R, int nf, const double* b) {
  for (int i = 0; i < nf; i++) {
    double s = 0.0;
    for (int k = 0; k < i; k++) s += R[i * nf + k] * x[k];
    x[i] = (b[i] + -s) / R[i * nf + i];
  }
  for (int i = nf - 1; i >= 0; i--) {
    double s = 0.0;
    for (int k = i + 1; k < nf; k++) s += R[k * nf + i] * x[k];
    x[i] = (x[i] + -s) / R[i * nf + i];
  }
}
double ClampTo(double v, double lo, double hi) { v = v < hi ? v : hi; return v > lo ? v : lo; }
double QPValue(const double* H, const double* g, int n, const double* x) {
  double q = 0.0, l = 0.0;
  for (int i = 0; i < n; i++) {
    double s = 0.0;
    for (int j = 0; j < n; j++) s += H[i * n + j] * x[j];
    q += x[i] * s;
    l += x[i] * g[i];
  }
  return 0.5 * q + l;
}
}  // namespace

void BoxQP::Allocate(int n) {
  res.assign(n, 0.0); R.assign((size_t)n * n, 0.0); H.assign((size_t)n * n, 0.0); g.assign(n, 0.0); lower.assign(n, 0.0); upper.assign(n, 0.0);
  index.assign(n, 0);
}

int BoxQPSolve(double* res, double* R, int* index, const double* H, const double* g, int n, const double* lower, const double* upper) {
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<double> buf(6 * (size_t)n);
  std::vector<int> mask(n, -1);
  double *grad = buf.data(), *search = grad + n, *cand = search + n, *y = cand + n, *lo = y + n, *hi = lo + n;
  for (int i = 0; i < n; i++) { lo[i] = lower ? lower[i] : -inf; hi[i] = upper ? upper[i] : inf; res[i] = ClampTo(res[i], lo[i], hi[i]); }
  double value = QPValue(H, g, n, res);
  int nf = 0;
  for (int iter = 0; iter < 100; iter++) {
    bool changed = false;
    nf = 0;
    for (int i = 0; i < n; i++) {
      double s = 0.0;
      for (int j = 0; j < n; j++) s += H[i * n + j] * res[j];
      grad[i] = g[i] + s;
      const int c = (res[i] == lo[i] && grad[i] > 0) || (res[i] == hi[i] && grad[i] < 0);
      if (mask[i] != c) changed = true;
      mask[i] = c;
      if (!c) index[nf++] = i;
    }
    if (nf == 0) break;
    if (changed && !CholFactorSub(R, H, n, index, nf)) return -1;
    double gn = 0.0;
    for (int i = 0; i < nf; i++) gn += grad[index[i]] * grad[index[i]];
    if (gn < 1.0e-16) break;
    for (int i = 0; i < nf; i++) y[i] = grad[index[i]];
    CholSolveSub(y, R, nf, y);
    std::fill(search, search + n, 0.0);
    double sdotg = 0.0;
    for (int i = 0; i < nf; i++) { search[index[i]] = -y[i]; sdotg += -y[i] * grad[index[i]]; }
    if (!(sdotg < 0)) break;
    double step = 1.0, nv = value;
    bool accepted = false;
    while (step >= 1.0e-22) {
      for (int i = 0; i < n; i++) cand[i] = ClampTo(res[i] + step * search[i], lo[i], hi[i]);
      nv = QPValue(H, g, n, cand);
      if (nv + -value <= 0.1 * (step * sdotg)) { accepted = true; break; }
      step = step * 0.5;
    }
    if (!accepted) break;
    std::copy(cand, cand + n, res);
    value = nv;
  }
  return nf;
}

void iLQGPolicy::Allocate(const MjpcHipModel* model, int num_residual, int num_trace, int horizon, int representation_) {
  Allocate(model->nq, model->nv, model->na, model->nu, model->njnt, model->jnt_type, model->jnt_qposadr, model->jnt_dofadr, model->actuator_ctrlrange,
           num_residual, num_trace, horizon, representation_);
}
void iLQGPolicy::Allocate(int nq_, int nv_, int na_, int nu_, int njnt, const int* type, const int* qposadr, const int* dofadr, const double* range,
                          int num_residual, int num_trace, int horizon, int representation_) {
  nq = nq_; nv = nv_; na = na_; nu = nu_;
  const int ds = nq + nv + na, nd = 2 * nv + na;
  ctrlrange.assign(range, range + 2 * nu);
  jnt_type.assign(type, type + njnt); jnt_qposadr.assign(qposadr, qposadr + njnt); jnt_dofadr.assign(dofadr, dofadr + njnt);
  trajectory.horizon = horizon; trajectory.dim_state = ds; trajectory.dim_action = nu; trajectory.dim_residual = num_residual; trajectory.dim_trace = 3 * num_trace;
  trajectory.states.assign((size_t)ds * horizon, 0.0); trajectory.actions.assign((size_t)nu * horizon, 0.0); trajectory.times.assign(horizon, 0.0);
  trajectory.residual.assign((size_t)num_residual * horizon, 0.0); trajectory.costs.assign(horizon, 0.0); trajectory.trace.assign((size_t)3 * num_trace * horizon, 0.0);
  feedback_gain.assign((size_t)nu * nd * horizon, 0.0);
  action_improvement.assign((size_t)nu * horizon, 0.0);
  state_scratch.assign(ds, 0.0); action_scratch.assign(nu, 0.0); feedback_gain_scratch.assign((size_t)nu * nd, 0.0); state_interp.assign(ds, 0.0);
  representation = representation_;
}
void iLQGPolicy::Reset(int horizon, const double* initial_repeated_action) {
  const int nd = 2 * nv + na;
  const size_t H = std::min((size_t)horizon, trajectory.times.size());
  trajectory.horizon = (int)H;
  std::fill(trajectory.states.begin(), trajectory.states.end(), 0.0);
  for (size_t i = 0; i < H * nu; i++) trajectory.actions[i] = initial_repeated_action ? initial_repeated_action[i % nu] : 0.0;
  std::fill(trajectory.times.begin(), trajectory.times.end(), 0.0);
  std::fill(trajectory.residual.begin(), trajectory.residual.end(), 0.0);
  std::fill(trajectory.costs.begin(), trajectory.costs.end(), 0.0);
  std::fill(trajectory.trace.begin(), trajectory.trace.end(), 0.0);
  trajectory.total_return = 0.0; trajectory.failure = false;
  std::fill(feedback_gain.begin(), feedback_gain.begin() + H * nu * nd, 0.0);
  std::fill(action_improvement.begin(), action_improvement.begin() + H * nu, 0.0);
  std::fill(state_scratch.begin(), state_scratch.end(), 0.0); std::fill(action_scratch.begin(), action_scratch.end(), 0.0);
  std::fill(feedback_gain_scratch.begin(), feedback_gain_scratch.end(), 0.0); std::fill(state_interp.begin(), state_interp.end(), 0.0);
  feedback_scaling = 1.0;
}
void StateDiff(const iLQGPolicy& p, double* ds, const double* s1, const double* s2, double h) {
  const int nq = p.nq, nv = p.nv, na = p.na;
  if (nq == nv) { for (int i = 0; i < nq + nv + na; i++) ds[i] = (s2[i] - s1[i]) / h; return; }
  // mj_differentiatePos: per joint, (qb - qa) / h, and for a quaternion the body-frame rotation vector of qa^-1 qb over h (mju_subQuat)
  auto quat = [&](double* res, const double* qa, const double* qb) {
    const double d[4] = {qa[0] * qb[0] + qa[1] * qb[1] + qa[2] * qb[2] + qa[3] * qb[3],
                         qa[0] * qb[1] - qa[1] * qb[0] - qa[2] * qb[3] + qa[3] * qb[2],
                         qa[0] * qb[2] + qa[1] * qb[3] - qa[2] * qb[0] - qa[3] * qb[1],
                         qa[0] * qb[3] - qa[1] * qb[2] + qa[2] * qb[1] - qa[3] * qb[0]};     // conj(qa) * qb
    double axis[3] = {d[1], d[2], d[3]};
    const double sn = std::sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]);
    if (sn < 1e-15) { axis[0] = 1.0; axis[1] = 0.0; axis[2] = 0.0; }        // mju_normalize3 of a zero vector
    else for (double& a : axis) a /= sn;
    double speed = 2 * atan2_cr(sn, d[0]);        // csrc/atan2_cr.h: the function the feedback rollout kernel evaluates (a library atan2 is a last place off between host and device)
    if (speed > M_PI) speed -= 2 * M_PI;
    for (int k = 0; k < 3; k++) res[k] = axis[k] * speed / h;
  };
  for (size_t j = 0; j < p.jnt_type.size(); j++) {
    const int qa = p.jnt_qposadr[j], da = p.jnt_dofadr[j];
    if (p.jnt_type[j] == 0) {
      for (int k = 0; k < 3; k++) ds[da + k] = (s2[qa + k] - s1[qa + k]) / h;
      quat(ds + da + 3, s1 + qa + 3, s2 + qa + 3);
    } else if (p.jnt_type[j] == 1) quat(ds + da, s1 + qa, s2 + qa);
    else ds[da] = (s2[qa] - s1[qa]) / h;
  }
  for (int i = 0; i < nv + na; i++) ds[nv + i] = (s2[nq + i] - s1[nq + i]) / h;
}
void iLQGPolicy::Action(double* action, const double* state, double time) const {
  const int ds = nq + nv + na, nd = 2 * nv + na, H = trajectory.horizon;
  int bounds[2];
  FindInterval(bounds, trajectory.times, time, H);
  auto normalize = [&]() {          // mj_normalizeQuat
    for (size_t j = 0; j < jnt_type.size(); j++) {
      if (jnt_type[j] > 1) continue;
      double* q = state_interp.data() + jnt_qposadr[j] + (jnt_type[j] == 0 ? 3 : 0);
      const double nrm = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
      if (nrm < 1e-15) { q[0] = 1.0; q[1] = q[2] = q[3] = 0.0; }
      else for (int k = 0; k < 4; k++) q[k] /= nrm;
    }
  };
  if (bounds[0] == bounds[1] || representation == kZeroSpline) {
    ZeroInterpolation(action, time, trajectory.times, trajectory.actions.data(), nu, H - 1);
    if (state) {
      ZeroInterpolation(state_interp.data(), time, trajectory.times, trajectory.states.data(), ds, H);
      ZeroInterpolation(feedback_gain_scratch.data(), time, trajectory.times, feedback_gain.data(), nu * nd, H - 1);
    }
  } else if (representation == kLinearSpline) {
    LinearInterpolation(action, time, trajectory.times, trajectory.actions.data(), nu, H - 1);
    if (state) {
      LinearInterpolation(state_interp.data(), time, trajectory.times, trajectory.states.data(), ds, H);
      normalize();
      LinearInterpolation(feedback_gain_scratch.data(), time, trajectory.times, feedback_gain.data(), nu * nd, H - 1);
    }
  } else if (representation == kCubicSpline) {
    CubicInterpolation(action, time, trajectory.times, trajectory.actions.data(), nu, H - 1);
    if (state) {
      CubicInterpolation(state_interp.data(), time, trajectory.times, trajectory.states.data(), ds, H);
      normalize();
      CubicInterpolation(feedback_gain_scratch.data(), time, trajectory.times, feedback_gain.data(), nu * nd, H - 1);
    }
  }
  if (state) {
    StateDiff(*this, state_scratch.data(), state_interp.data(), state, 1.0);
    for (int i = 0; i < nu; i++) {
      double s = 0.0;
      for (int j = 0; j < nd; j++) s += feedback_gain_scratch[(size_t)i * nd + j] * state_scratch[j];
      action[i] += s * feedback_scaling;
    }
  }
  for (int i = 0; i < nu; i++) action[i] = std::max(ctrlrange[2 * i], std::min(ctrlrange[2 * i + 1], action[i]));
}
void iLQGPolicy::CopyFrom(const iLQGPolicy& policy, int horizon) {
  trajectory = policy.trajectory;
  const int nd = 2 * nv + na;
  std::copy(policy.feedback_gain.begin(), policy.feedback_gain.begin() + std::min((size_t)horizon * nu * nd, policy.feedback_gain.size()), feedback_gain.begin());
  std::copy(policy.action_improvement.begin(), policy.action_improvement.begin() + std::min((size_t)horizon * nu, policy.action_improvement.size()), action_improvement.begin());
}

void iLQGBackwardPass::Allocate(int n, int m, int T) {
  const size_t Tz = T, T1 = T > 1 ? T - 1 : 0, mmn = std::max(n, m);
  Vx.assign(n * Tz, 0.0); Vxx.assign((size_t)n * n * Tz, 0.0);
  Qx.assign(n * T1, 0.0); Qu.assign(m * T1, 0.0); Qxx.assign((size_t)n * n * T1, 0.0); Qxu.assign((size_t)n * m * T1, 0.0); Quu.assign((size_t)m * m * T1, 0.0);
  Q_scratch.assign(10 * ((size_t)n * n + 7 * m + 2 * (size_t)m * m + (size_t)n * m + 3 * mmn * mmn), 0.0);
  regularization = 1.0; regularization_rate = 1.0; regularization_factor = 2.0;
}
void iLQGBackwardPass::Reset(int n, int m, int T) {
  const size_t Tz = T;
  if (Vx.size() < n * Tz || Vxx.size() < (size_t)n * n * Tz || Qu.size() + m < m * Tz || Qxu.size() + (size_t)n * m < (size_t)n * m * Tz ||
      Quu.size() + (size_t)m * m < (size_t)m * m * Tz) Allocate(n, m, T);
  dV[0] = 0.0; dV[1] = 0.0;
  for (std::vector<double>* v : {&Vx, &Vxx, &Qx, &Qu, &Qxx, &Qxu, &Quu}) std::fill(v->begin(), v->end(), 0.0);
  regularization = 1.0; regularization_rate = 1.0; regularization_factor = 2.0;
}

int iLQGBackwardPass::RiccatiStep(int n, int m, double mu, const double* Wx, const double* Wxx, const double* At, const double* Bt, const double* cxt,
                                  const double* cut, const double* cxxt, const double* cxut, const double* cuut, double* Vxt, double* Vxxt, double* dut,
                                  double* Kt, double* dV_, double* Qxt, double* Qut, double* Qxxt, double* Qxut, double* Quut, double* scratch,
                                  BoxQP& boxqp, const double* action, const double* action_limits, int reg_type, int limits) {
  const int mmn = std::max(m, n);
  double* Vxx_reg = scratch; scratch += n * n;
  double* Quu_reg = scratch; scratch += m * m;
  double* tmp = scratch; scratch += mmn * mmn;
  double* tmp2 = scratch; scratch += mmn * mmn;
  double* tmp3 = scratch; scratch += mmn * mmn;
  std::vector<int> identity;

  // Qx, Qxx, Qu, Qxu, Quu
  MulMatTMat(tmp, At, Wxx, n, n, n);
  MulMatTMat(Qxt, At, Wx, n, n, 1);
  for (int i = 0; i < n; i++) Qxt[i] += cxt[i];
  MulMatMat(Qxxt, tmp, At, n, n, n);
  for (int i = 0; i < n * n; i++) Qxxt[i] += cxxt[i];
  MulMatTMat(Qut, Bt, Wx, n, m, 1);
  for (int i = 0; i < m; i++) Qut[i] += cut[i];
  MulMatMat(Qxut, tmp, Bt, n, n, m);
  for (int i = 0; i < n * m; i++) Qxut[i] += cxut[i];
  MulMatTMat(tmp2, Bt, Wxx, n, m, n);
  MulMatMat(Quut, tmp2, Bt, m, n, m);
  for (int i = 0; i < m * m; i++) Quut[i] += cuut[i];

  // regularise (Qxu_reg, which the reference forms and never reads, is not formed)
  if (reg_type == kValueRegularization) {
    std::copy(Wxx, Wxx + n * n, Vxx_reg);
    for (int i = 0; i < n; i++) Vxx_reg[n * i + i] += mu;
    MulMatTMat(tmp2, Bt, Vxx_reg, n, m, n);
    MulMatMat(Quu_reg, tmp2, Bt, m, n, m);
    for (int i = 0; i < m * m; i++) Quu_reg[i] += cuut[i];
  } else {
    std::copy(Quut, Quut + m * m, Quu_reg);
  }
  if (mu) {
    if (reg_type == kControlRegularization) {
      for (int i = 0; i < m; i++) Quu_reg[i * m + i] += mu;
    } else if (reg_type == kStateControlRegularization) {
      MulMatTMat(tmp, Bt, Bt, n, m, m);
      for (int i = 0; i < m * m; i++) Quu_reg[i] += tmp[i] * mu;
    }
  }

  std::fill(Kt, Kt + n * m, 0.0);
  int mFree = m;
  const int* index = nullptr;
  const double* R = nullptr;
  if (limits == 1) {
    std::copy(Quu_reg, Quu_reg + m * m, boxqp.H.begin());
    std::copy(Qut, Qut + m, boxqp.g.begin());
    for (int i = 0; i < m; i++) {
      boxqp.lower[i] = action_limits[2 * i] - action[i];
      boxqp.upper[i] = action_limits[2 * i + 1] - action[i];
    }
    mFree = BoxQPSolve(boxqp.res.data(), boxqp.R.data(), boxqp.index.data(), boxqp.H.data(), boxqp.g.data(), m, boxqp.lower.data(), boxqp.upper.data());
    if (mFree < 0) return 0;
    index = boxqp.index.data(); R = boxqp.R.data();
    std::copy(boxqp.res.begin(), boxqp.res.begin() + m, dut);
  } else {
    identity.resize(m);
    for (int i = 0; i < m; i++) identity[i] = i;
    if (!CholFactorSub(tmp3, Quu_reg, m, identity.data(), m)) return 0;        // "backward pass failure": rank below m
    index = identity.data(); R = tmp3;
    CholSolveSub(dut, R, m, Qut);
    for (int i = 0; i < m; i++) dut[i] = -dut[i];
  }
  // K = -H_free \ Qxu_free', zero rows for the clamped controls (the UNREGULARISED Qxu, as the reference)
  for (int j = 0; j < n; j++) {
    double* y = tmp + (size_t)j * m;
    for (int i = 0; i < mFree; i++) y[i] = Qxut[j * m + index[i]];
    CholSolveSub(y, R, mFree, y);
    for (int i = 0; i < mFree; i++) Kt[index[i] * n + j] = -y[i];
  }

  // cost-to-go
  double d0 = 0.0, d1 = 0.0;
  for (int i = 0; i < m; i++) d0 += dut[i] * Qut[i];
  dV_[0] += d0;
  MulMatMat(tmp, Quut, dut, m, m, 1);
  for (int i = 0; i < m; i++) d1 += dut[i] * tmp[i];
  dV_[1] += 0.5 * d1;
  for (int i = 0; i < m; i++) tmp2[i] = tmp[i] + Qut[i];
  MulMatTMat(tmp, Kt, tmp2, m, n, 1);
  for (int i = 0; i < n; i++) Vxt[i] = Qxt[i] + tmp[i];
  MulMatMat(tmp, Qxut, dut, n, m, 1);
  for (int i = 0; i < n; i++) Vxt[i] += tmp[i];
  MulMatMat(tmp2, Quut, Kt, m, m, n);               // Quu K
  MulMatTMat(tmp3, Kt, tmp2, m, n, n);              // K' Quu K
  for (int i = 0; i < n * n; i++) Vxxt[i] = Qxxt[i] + tmp3[i];
  MulMatMat(tmp2, Qxut, Kt, n, m, n);               // Qxu K
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) tmp[i * n + j] = tmp2[i * n + j] + tmp2[j * n + i];
  for (int i = 0; i < n * n; i++) Vxxt[i] += tmp[i];
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) tmp[i * n + j] = 0.5 * (Vxxt[i * n + j] + Vxxt[j * n + i]);
  std::copy(tmp, tmp + n * n, Vxxt);
  return 1;
}

int iLQGBackwardPass::Riccati(iLQGPolicy* p, const ModelDerivatives* md, const CostDerivatives* cd, int n, int m, int T, double reg, BoxQP& boxqp,
                              const double* actions, const double* action_limits, const iLQGSettings& settings) {
  if (T < 2) { Fatal("iLQGBackwardPass: T < 2"); return -1; }
  const size_t nn = (size_t)n * n, nm = (size_t)n * m, mm = (size_t)m * m;
  dV[0] = 0.0; dV[1] = 0.0;
  std::copy(cd->cx.begin() + (size_t)(T - 1) * n, cd->cx.begin() + (size_t)T * n, Vx.begin() + (size_t)(T - 1) * n);
  std::copy(cd->cxx.begin() + (T - 1) * nn, cd->cxx.begin() + T * nn, Vxx.begin() + (T - 1) * nn);
  int bp_iter = 0, time_index = T - 1;
  while (bp_iter < settings.max_regularization_iterations) {
    for (int t = T - 1; t > 0; t--) {
      const size_t u = t - 1;
      const int status = RiccatiStep(n, m, reg, Vx.data() + (size_t)t * n, Vxx.data() + t * nn, md->A.data() + u * nn, md->B.data() + u * nm,
                                     cd->cx.data() + u * n, cd->cu.data() + u * m, cd->cxx.data() + u * nn, cd->cxu.data() + u * nm, cd->cuu.data() + u * mm,
                                     Vx.data() + u * n, Vxx.data() + u * nn, p->action_improvement.data() + u * m, p->feedback_gain.data() + u * nm, dV,
                                     Qx.data() + u * n, Qu.data() + u * m, Qxx.data() + u * nn, Qxu.data() + u * nm, Quu.data() + u * mm, Q_scratch.data(),
                                     boxqp, actions + u * m, action_limits, settings.regularization_type, settings.action_limits);
      if (!status) { time_index = t - 1; break; }
      if (t == 1) {
        std::copy(p->feedback_gain.begin() + (T - 2) * nm, p->feedback_gain.begin() + (T - 1) * nm, p->feedback_gain.begin() + (T - 1) * nm);
        std::copy(p->action_improvement.begin() + (size_t)(T - 2) * m, p->action_improvement.begin() + (size_t)(T - 1) * m, p->action_improvement.begin() + (size_t)(T - 1) * m);
        return 0;
      }
    }
    if (regularization <= settings.max_regularization) {
      ScaleRegularization(regularization_factor, settings.min_regularization, settings.max_regularization);
      bp_iter += 1;
    } else {
      return time_index;
    }
  }
  return time_index;
}

void iLQGBackwardPass::RiccatiRegularized(double* k, double* K, const double* A, const double* B, const double* cx, const double* cu, const double* cxx,
                                          const double* cxu, const double* cuu, int n, int m, int T, BoxQP& boxqp, const double* actions,
                                          const double* action_limits, const iLQGSettings& settings, int* status) {
  if (T < 2) { Fatal("iLQGBackwardPass: T < 2"); return; }
  const size_t nn = (size_t)n * n, nm = (size_t)n * m, mm = (size_t)m * m;
  if (Vx.size() < (size_t)n * T || Vxx.size() < nn * T || Qx.size() < (size_t)n * (T - 1) || Qu.size() < (size_t)m * (T - 1) || Qxx.size() < nn * (T - 1) ||
      Qxu.size() < nm * (T - 1) || Quu.size() < mm * (T - 1) || Q_scratch.empty()) {
    const double r = regularization, rr = regularization_rate, f = regularization_factor;
    Allocate(n, m, T);
    regularization = r; regularization_rate = rr; regularization_factor = f;
  }
  if ((int)boxqp.res.size() < m) boxqp.Allocate(m);
  std::fill(boxqp.res.begin(), boxqp.res.end(), 0.0);
  int iter = 0, done = 0, failed = -1;
  dV[0] = 0.0; dV[1] = 0.0;
  std::copy(cx + (size_t)(T - 1) * n, cx + (size_t)T * n, Vx.begin() + (size_t)(T - 1) * n);
  std::copy(cxx + (T - 1) * nn, cxx + T * nn, Vxx.begin() + (T - 1) * nn);
  while (iter < settings.max_regularization_iterations && !done) {
    dV[0] = 0.0; dV[1] = 0.0;
    failed = -1;
    for (int t = T - 2; t >= 0; t--) {
      const size_t u = t;
      const int ok = RiccatiStep(n, m, regularization, Vx.data() + (u + 1) * n, Vxx.data() + (u + 1) * nn, A + u * nn, B + u * nm, cx + u * n, cu + u * m,
                                 cxx + u * nn, cxu + u * nm, cuu + u * mm, Vx.data() + u * n, Vxx.data() + u * nn, k + u * m, K + u * nm, dV,
                                 Qx.data() + u * n, Qu.data() + u * m, Qxx.data() + u * nn, Qxu.data() + u * nm, Quu.data() + u * mm, Q_scratch.data(),
                                 boxqp, actions ? actions + u * m : nullptr, action_limits, settings.regularization_type, settings.action_limits);
      if (!ok) { failed = t; break; }
    }
    if (failed < 0) {
      done = 1;
      std::copy(K + (T - 2) * nm, K + (T - 1) * nm, K + (T - 1) * nm);
      std::copy(k + (size_t)(T - 2) * m, k + (size_t)(T - 1) * m, k + (size_t)(T - 1) * m);
    } else if (regularization <= settings.max_regularization) {
      ScaleRegularization(regularization_factor, settings.min_regularization, settings.max_regularization);
      iter += 1;
    } else {
      break;         // (the reference's loop would neither scale nor count from here on)
    }
  }
  if (status) { status[0] = done; status[1] = done ? -1 : failed; status[2] = iter; }
}

static MjpcHipRiccatiSettings RiccatiSettingsOf(const iLQGSettings& s, double factor) {
  MjpcHipRiccatiSettings r;
  r.struct_size = (int)sizeof(MjpcHipRiccatiSettings);
  r.regularization_type = s.regularization_type; r.action_limits = s.action_limits; r.max_regularization_iterations = s.max_regularization_iterations;
  r.min_regularization = s.min_regularization; r.max_regularization = s.max_regularization; r.regularization_factor = factor;
  return r;
}

bool iLQGBackwardPass::Compute(MjpcHipEngine* engine, iLQGPolicy* policy, const ModelDerivatives* md, const CostDerivatives* cd, int n, int m, int T,
                               const double* actions, const double* action_limits, const iLQGSettings& settings, int* status) {
  const double r = regularization, rr = regularization_rate, f = regularization_factor;
  Reset(n, m, T);
  regularization = r; regularization_rate = rr; regularization_factor = f;
  const MjpcHipRiccatiSettings s = RiccatiSettingsOf(settings, regularization_factor);
  return mjpc_hip_ilqg_backward_pass(engine, T, n, m, md->A.data(), md->B.data(), cd->cx.data(), cd->cu.data(), cd->cxx.data(), cd->cxu.data(), cd->cuu.data(),
                                     actions, action_limits, &s, &regularization, &regularization_rate, policy->action_improvement.data(),
                                     policy->feedback_gain.data(), Vx.data(), Vxx.data(), Qx.data(), Qu.data(), Qxx.data(), Qxu.data(), Quu.data(), dV, status) == 0;
}

bool iLQGBackwardPass::ComputeFused(MjpcHipEngine* engine, iLQGPolicy* policy, const double* x, const double* u, const double* h, const double* residual,
                                    int n, int m, int T, const iLQGSettings& settings, int* status, int* failure, const double* mocap, const double* userdata) {
  const double r = regularization, rr = regularization_rate, f = regularization_factor;
  Reset(n, m, T);
  regularization = r; regularization_rate = rr; regularization_factor = f;
  const MjpcHipRiccatiSettings s = RiccatiSettingsOf(settings, regularization_factor);
  return mjpc_hip_trajectory_ilqg(engine, T, x, u, h, residual, mocap, userdata, settings.fd_tolerance, settings.fd_mode != 0 ? 1 : 0, &s, &regularization,
                                  &regularization_rate, policy->action_improvement.data(), policy->feedback_gain.data(), Vx.data(), Vxx.data(), Qx.data(),
                                  Qu.data(), Qxx.data(), Qxu.data(), Quu.data(), dV, status, failure) == 0;
}

void iLQGBackwardPass::ScaleRegularization(double factor, double reg_min, double reg_max) {
  const double s = regularization_rate * factor;
  if (factor > 1) regularization_rate = s > factor ? s : factor;
  else regularization_rate = s < factor ? s : factor;
  double v = regularization * regularization_rate;
  v = v > reg_min ? v : reg_min;
  regularization = v < reg_max ? v : reg_max;
}

void iLQGBackwardPass::UpdateRegularization(double reg_min, double reg_max, double z, double s) {
  auto bad = [](double v) { return std::isnan(v) || v > 1e10 || v < -1e10; };          // mju_isBad: NaN or beyond mjMAXVAL
  if (bad(z) || bad(s)) ScaleRegularization(regularization_factor * regularization_factor, reg_min, reg_max);
  else if (z > 0.5 || s > 0.3) ScaleRegularization(1.0 / regularization_factor, reg_min, reg_max);
  else if (z < 0.1 || s < 0.06) ScaleRegularization(regularization_factor, reg_min, reg_max);
}

// ------------------------------------------------------------------ iLQGPlanner (ilqg/planner.cc:40-729)
iLQGPlanner::~iLQGPlanner() { if (engine_) mjpc_hip_destroy(engine_); }

void iLQGPlanner::Initialize(const MjpcHipModel* model, const MjpcHipTask* task, const Numerics& numerics) {
  numerics_ = numerics;
  ns_ = model->nq + model->nv + model->na; nd_ = 2 * model->nv + model->na; nu_ = model->nu; nr_ = task->num_residual; ntrace_ = task->num_trace;
  nmocap_ = model->nmocap; nuserdata_ = model->nuserdata;
  derivative_skip_ = numerics.derivative_skip;
  if (representation < kZeroSpline || representation > kCubicSpline) { Fatal("Unknown ilqg_representation"); return; }
  if (num_trajectory < 1 || num_trajectory > kMaxiLQGTrajectory) { Fatal("Too many trajectories."); return; }
  if (engine_) { mjpc_hip_destroy(engine_); engine_ = nullptr; }
  engine_ = mjpc_hip_create(model, task, std::max(numerics.max_samples, num_trajectory), std::max(numerics.max_horizon, 2), numerics.device);
  if (!engine_) { Fatal(mjpc_hip_last_error()); return; }
  ctrlrange_.assign(model->actuator_ctrlrange, model->actuator_ctrlrange + 2 * nu_);
  for (iLQGPolicy* p : {&policy, &previous_policy, &candidate}) p->Allocate(model, nr_, ntrace_, numerics.max_horizon, representation);
}

void iLQGPlanner::Allocate() {
  if (!engine_) return;
  const size_t Hm = (size_t)numerics_.max_horizon;
  state.assign(ns_, 0.0); mocap.assign(7 * nmocap_, 0.0); userdata.assign(nuserdata_, 0.0);
  Trajectory* tr = &trajectory_winner;
  tr->dim_state = ns_; tr->dim_action = nu_; tr->dim_residual = nr_; tr->dim_trace = 3 * ntrace_;
  tr->states.assign(Hm * ns_, 0.0); tr->actions.assign(Hm * nu_, 0.0); tr->times.assign(Hm, 0.0); tr->residual.assign(Hm * nr_, 0.0);
  tr->costs.assign(Hm, 0.0); tr->trace.assign(Hm * 3 * std::max(ntrace_, 1), 0.0);
  // (the policies' trajectories were sized by iLQGPolicy::Allocate with dim_trace = 3 ntrace: give the trace row one element at least)
  for (iLQGPolicy* p : {&policy, &previous_policy, &candidate}) if (p->trajectory.trace.empty()) p->trajectory.trace.assign(Hm, 0.0);
  model_derivative.Allocate(nd_, nu_, nr_, (int)Hm, ns_);
  cost_derivative.Allocate(nd_, nu_, nr_, (int)Hm);
  backward_pass.Allocate(nd_, nu_, (int)Hm);
  const size_t N = (size_t)std::max(numerics_.max_samples, num_trajectory);
  zeros_.assign(N, 0.0); ones_.assign(N, 1.0); fail_.assign(Hm, 0);
  winner = -1;
}

void iLQGPlanner::Reset(int horizon, const double* initial_repeated_action) {
  std::fill(state.begin(), state.end(), 0.0); std::fill(mocap.begin(), mocap.end(), 0.0); std::fill(userdata.begin(), userdata.end(), 0.0);
  time = 0.0;
  const int h = horizon > 0 ? std::min(horizon, numerics_.max_horizon) : numerics_.max_horizon;
  model_derivative.Reset(nd_, nu_, nr_, h); cost_derivative.Reset(nd_, nu_, nr_, h); backward_pass.Reset(nd_, nu_, h);
  for (iLQGPolicy* p : {&policy, &previous_policy, &candidate}) { p->Reset(h, initial_repeated_action); p->representation = representation; }
  feedback_scaling = 1.0; action_step = 0.0; expected = 0.0; improvement = 0.0; surprise = 0.0;
  winner = -1; backward_pass_failed = false; all_failed = false; adopted = false;
  derivative_skip_ = numerics_.derivative_skip;
}

void iLQGPlanner::SetState(const double* s, const double* m, const double* u, double t) {
  std::copy(s, s + ns_, state.begin());
  if (m) std::copy(m, m + 7 * nmocap_, mocap.begin());
  if (u) std::copy(u, u + nuserdata_, userdata.begin());
  time = t;
}

void iLQGPlanner::SetTask(const MjpcHipTask* task) { if (mjpc_hip_set_task(engine_, task) != 0) Fatal(mjpc_hip_last_error()); }

void iLQGPlanner::ActionFromPolicy(double* action, const double* s, double t, bool use_previous) {
  const std::shared_lock<std::shared_mutex> lock(mtx_);
  (use_previous ? previous_policy : policy).Action(action, s, t);
}

int iLQGPlanner::BestRollout(const double* ret, const int* fail, int n) {
  double best_return = 0; int best_rollout = -1;
  for (int j = n - 1; j >= 0; j--) {
    if (fail[j]) continue;
    if (best_rollout == -1 || ret[j] < best_return) { best_return = ret[j]; best_rollout = j; }
  }
  return best_rollout;
}

void iLQGPlanner::LogScale(double* values, double max_value, double min_value, int steps) {   // utilities.cc:802-808
  const double step = (std::log(max_value) - std::log(min_value)) / std::max((steps - 1), 1);
  for (int i = 0; i < steps; i++) values[i] = std::exp(std::log(min_value) + i * step);       // ascending, as the reference spells it: no pinned value
}

bool iLQGPlanner::Rollouts(const iLQGPolicy& p, int mode, int horizon, const double* alpha, const double* scale, bool use_feedback, bool improvement_term) {
  const int N = num_trajectory;
  returns.assign(N, 0.0); failures.assign(N, 0);
  MjpcHipPlanInput in;
  std::memset(&in, 0, sizeof(in));
  in.state = state.data(); in.mocap = mocap.data(); in.userdata = userdata.data(); in.time = time;
  in.num_trajectory = N; in.num_local = N; in.horizon = horizon;
  MjpcHipFeedbackPolicy fp;
  std::memset(&fp, 0, sizeof(fp));
  fp.struct_size = (int)sizeof(fp); fp.mode = mode; fp.T = horizon; fp.representation = p.representation;
  fp.times = p.trajectory.times.data(); fp.states = p.trajectory.states.data(); fp.actions = p.trajectory.actions.data();
  fp.feedback_gain = p.feedback_gain.data(); fp.action_improvement = improvement_term ? p.action_improvement.data() : nullptr;
  fp.action_step = alpha; fp.feedback_scaling = scale; fp.use_feedback = use_feedback ? 1 : 0;
  MjpcHipPlanOutput out;
  std::memset(&out, 0, sizeof(out));
  out.returns = returns.data(); out.failure = failures.data();
  const int rc = mjpc_hip_plan_feedback(engine_, &in, &fp, &out);
  if (rc != 0 && rc != -3) { Fatal(mjpc_hip_last_error()); return false; }               // -3: no finite return; returns[] / failure[] are valid
  rollout_kernel_time = out.rollouts_compute_time_us;
  return true;
}

bool iLQGPlanner::Fetch(int index, int horizon, Trajectory& tr) {
  MjpcHipPlanOutput out;
  std::memset(&out, 0, sizeof(out));
  out.states = tr.states.data(); out.actions = tr.actions.data(); out.times = tr.times.data();
  out.residual = tr.residual.data(); out.costs = tr.costs.data(); out.trace = tr.trace.data();
  if (mjpc_hip_get_candidate(engine_, index, &out) != 0) { Fatal(mjpc_hip_last_error()); return false; }
  // trajectory.cc: the last action repeats the one before it (the kernel applies none at the terminal step)
  if (horizon > 1) std::copy(tr.actions.begin() + (size_t)(horizon - 2) * nu_, tr.actions.begin() + (size_t)(horizon - 1) * nu_, tr.actions.begin() + (size_t)(horizon - 1) * nu_);
  tr.horizon = horizon; tr.total_return = returns[index]; tr.failure = failures[index] != 0;
  return true;
}

bool iLQGPlanner::NominalTrajectory(int horizon) {   // planner.cc:167-223
  using clock = std::chrono::steady_clock;
  nominal_ok_ = false;
  if (!engine_ || num_trajectory == 0) return false;
  if (horizon < 2 || horizon > numerics_.max_horizon) { Fatal("iLQGPlanner: horizon out of range (2 .. max_horizon)"); return false; }
  auto t0 = clock::now();
  num_trajectory = std::max(1, std::min(num_trajectory, std::min(numerics_.max_samples, kMaxiLQGTrajectory)));
  const int N = num_trajectory;
  policy.trajectory.horizon = horizon;
  linesearch_steps.assign(N, 0.0);
  if (N > 1) LogScale(linesearch_steps.data(), 1.0, settings.min_linesearch_step, N - 1);
  linesearch_steps[N - 1] = 0.0;
  { const std::shared_lock<std::shared_mutex> lock(mtx_); candidate.CopyFrom(policy, horizon); candidate.representation = policy.representation; }
  // FeedbackRollouts: the policy interpolated at the step's time, feedback scale = the step
  if (!Rollouts(candidate, MJPC_FEEDBACK_TIME, horizon, zeros_.data(), linesearch_steps.data(), settings.nominal_feedback_scaling != 0, false)) return false;
  resample_kernel_time = mjpc_hip_feedback_resample_time_us(engine_);
  const int best = BestRollout(returns.data(), failures.data(), N);
  all_failed = best == -1;
  if (best == -1) {
    const std::shared_lock<std::shared_mutex> lock(mtx_);
    candidate.trajectory = policy.trajectory;
    feedback_scaling = 0.0;
  } else {
    Fetch(best, horizon, candidate.trajectory);
    feedback_scaling = linesearch_steps[best];
  }
  nominal_compute_time = std::chrono::duration<double, std::micro>(clock::now() - t0).count();
  nominal_ok_ = true; nominal_horizon_ = horizon;
  return true;
}

void iLQGPlanner::Iteration(int horizon) {   // planner.cc:377-615
  using clock = std::chrono::steady_clock;
  auto us = [](clock::time_point t0) { return std::chrono::duration<double, std::micro>(clock::now() - t0).count(); };
  adopted = false;
  // only behind a NominalTrajectory (or SetNominal) of the same horizon and batch that went through: it sized linesearch_steps and filled `candidate`
  if (!engine_ || !nominal_ok_ || horizon != nominal_horizon_ || num_trajectory < 1 || (int)linesearch_steps.size() != num_trajectory) {
    if (engine_) Fatal("iLQGPlanner::Iteration: no nominal trajectory of this horizon and batch (call NominalTrajectory first)");
    return;
  }
  const int N = num_trajectory;
  const double previous_return = candidate.trajectory.total_return;
  if (N > 1) LogScale(linesearch_steps.data(), 1.0, settings.min_linesearch_step, N - 1);
  linesearch_steps[N - 1] = 0.0;
  derivative_compute_time = rollouts_compute_time = policy_update_compute_time = 0.0;
  backward_pass_failed = false; adopted = false;

  // ----- derivatives and backward pass of the nominal -----
  auto t0 = clock::now();
  const Trajectory& tr = candidate.trajectory;
  std::fill(fail_.begin(), fail_.end(), 0);
  bool ok;
  if (fused && derivative_skip_ <= 0) {
    ok = backward_pass.ComputeFused(engine_, &candidate, tr.states.data(), tr.actions.data(), tr.times.data(), tr.residual.data(), nd_, nu_, horizon, settings,
                                    backward_pass_status, fail_.data(), mocap.data(), userdata.data());
  } else {
    ok = model_derivative.Compute(engine_, tr.states.data(), tr.actions.data(), tr.times.data(), horizon, settings.fd_tolerance, settings.fd_mode != 0 ? 1 : 0,
                                  derivative_skip_, mocap.data(), userdata.data()) &&
         cost_derivative.Compute(engine_, tr.residual.data(), model_derivative.C.data(), model_derivative.D.data(), nd_, nu_, nr_, horizon, true);
    if (ok) {
      std::copy(model_derivative.failure.begin(), model_derivative.failure.begin() + horizon, fail_.begin());
      ok = backward_pass.Compute(engine_, &candidate, &model_derivative, &cost_derivative, nd_, nu_, horizon, tr.actions.data(), ctrlrange_.data(), settings,
                                 backward_pass_status);
    }
  }
  derivative_compute_time = us(t0);
  if (!ok) { Fatal(mjpc_hip_last_error()); backward_pass_failed = true; return; }
  for (int t = 0; t < horizon; t++) if (fail_[t]) { backward_pass_failed = true; return; }     // a failed derivative evaluation: as a failed pass
  if (backward_pass_status[0] == 0) { backward_pass_failed = true; return; }                    // planner.cc:524-532: the policy stays as it was

  // ----- ActionRollouts: one batch, action step = the line-search step, full feedback -----
  t0 = clock::now();
  if (!Rollouts(candidate, MJPC_FEEDBACK_INDEXED, horizon, linesearch_steps.data(), ones_.data(), true, true)) return;
  const int best = BestRollout(returns.data(), failures.data(), N);
  if (best == -1) return;
  winner = best;
  if (!Fetch(winner, horizon, trajectory_winner)) return;
  // candidate_policy[winner] as the reference leaves it: the nominal with actions ubar + step k (mju_addScl over nu * horizon); slot 0
  // is the winning rollout itself by the time the policy is copied
  action_step = linesearch_steps[winner];
  if (winner == 0) candidate.trajectory = trajectory_winner;
  else for (size_t e = 0; e < (size_t)nu_ * horizon; e++) candidate.trajectory.actions[e] = candidate.trajectory.actions[e] + candidate.action_improvement[e] * action_step;
  expected = -1.0 * action_step * (backward_pass.dV[0] + action_step * backward_pass.dV[1]) + 1.0e-16;
  improvement = previous_return - trajectory_winner.total_return;
  surprise = std::min(std::max(0.0, improvement / expected), 2.0);
  backward_pass.UpdateRegularization(settings.min_regularization, settings.max_regularization, surprise, action_step);
  rollouts_compute_time = us(t0);

  // ----- policy update -----
  t0 = clock::now();
  {
    const std::unique_lock<std::shared_mutex> lock(mtx_);
    previous_policy = policy;
    policy.CopyFrom(candidate, horizon);
    policy.feedback_scaling = 1.0;
  }
  adopted = true;
  policy_update_compute_time = us(t0);
}

void iLQGPlanner::OptimizePolicy(int horizon) {
  if (!NominalTrajectory(horizon)) return;        // refused (horizon, engine error): the policy stays as it was
  Iteration(horizon);
}

bool iLQGPlanner::SetNominal(const Trajectory& tr, int horizon) {   // ilqs/planner.cc:198
  if (!engine_ || num_trajectory == 0) return false;
  if (horizon < 2 || horizon > numerics_.max_horizon) { Fatal("iLQGPlanner: horizon out of range (2 .. max_horizon)"); return false; }
  const size_t H = (size_t)horizon;
  if (tr.dim_state != ns_ || tr.dim_action != nu_ || tr.dim_residual != nr_ || tr.states.size() < H * ns_ || tr.actions.size() < H * nu_ ||
      tr.times.size() < H || tr.residual.size() < H * nr_) { Fatal("iLQGPlanner::SetNominal: the trajectory's dimensions are not this planner's"); return false; }
  num_trajectory = std::max(1, std::min(num_trajectory, std::min(numerics_.max_samples, kMaxiLQGTrajectory)));
  const int N = num_trajectory;
  linesearch_steps.assign(N, 0.0);
  if (N > 1) LogScale(linesearch_steps.data(), 1.0, settings.min_linesearch_step, N - 1);
  linesearch_steps[N - 1] = 0.0;
  Trajectory& c = candidate.trajectory;
  std::copy(tr.states.begin(), tr.states.begin() + H * ns_, c.states.begin());
  std::copy(tr.actions.begin(), tr.actions.begin() + H * nu_, c.actions.begin());
  std::copy(tr.times.begin(), tr.times.begin() + H, c.times.begin());
  std::copy(tr.residual.begin(), tr.residual.begin() + H * nr_, c.residual.begin());
  if (tr.costs.size() >= H) std::copy(tr.costs.begin(), tr.costs.begin() + H, c.costs.begin());
  // trajectory.cc: the last action repeats the one before it
  std::copy(c.actions.begin() + (H - 2) * nu_, c.actions.begin() + (H - 1) * nu_, c.actions.begin() + (H - 1) * nu_);
  c.horizon = horizon; c.total_return = tr.total_return; c.failure = tr.failure;
  policy.trajectory.horizon = horizon;
  nominal_ok_ = true; nominal_horizon_ = horizon;
  return true;
}

// ------------------------------------------------------------------ spline mappings (gradient/spline_mapping.cc)
void SplineMapping::Allocate(int d) {
  dim = d;
  mapping.assign((size_t)(dim * kMaxTrajectoryHorizon) * (dim * kMaxGradientSplinePoints), 0.0);
}
void ZeroSplineMapping::Compute(const std::vector<double>& input_times, int num_input, const double* output_times, int num_output) {
  std::fill(mapping.begin(), mapping.begin() + (size_t)(dim * num_output) * (dim * num_input), 0.0);
  int bounds[2];
  for (int i = 0; i < num_output; i++) {
    FindInterval(bounds, input_times, output_times[i], num_input);
    for (int j = 0; j < dim; j++) mapping[(size_t)dim * num_input * (dim * i + j) + dim * bounds[0] + j] = 1.0;
  }
}
void LinearSplineMapping::Compute(const std::vector<double>& input_times, int num_input, const double* output_times, int num_output) {
  std::fill(mapping.begin(), mapping.begin() + (size_t)(dim * num_output) * (dim * num_input), 0.0);
  int bounds[2];
  for (int i = 0; i < num_output; i++) {
    FindInterval(bounds, input_times, output_times[i], num_input);
    for (int j = 0; j < dim; j++) {
      const size_t row = (size_t)dim * num_input * (dim * i + j);
      if (bounds[0] == bounds[1]) { mapping[row + dim * bounds[0] + j] = 1.0; continue; }
      double a = (output_times[i] - input_times[bounds[0]]) / (input_times[bounds[1]] - input_times[bounds[0]]);
      mapping[row + dim * bounds[0] + j] = 1.0 - a;
      mapping[row + dim * bounds[1] + j] = a;
    }
  }
}
void CubicSplineMapping::Allocate(int d) {
  SplineMapping::Allocate(d);
  point_slope_mapping.assign((size_t)(2 * dim * kMaxGradientSplinePoints) * (dim * kMaxGradientSplinePoints), 0.0);
  output_mapping.assign((size_t)(dim * kMaxTrajectoryHorizon) * (2 * dim * kMaxGradientSplinePoints), 0.0);
}
void CubicSplineMapping::Compute(const std::vector<double>& input_times, int num_input, const double* output_times, int num_output) {
  const size_t ni = (size_t)dim * num_input;
  std::fill(point_slope_mapping.begin(), point_slope_mapping.begin() + 2 * ni * ni, 0.0);
  for (size_t r = 0; r < ni; r++) point_slope_mapping[ni * r + r] = 1.0;                  // point-to-point
  const size_t shift = ni * ni;                                                            // point-to-FiniteDifferenceSlope
  for (int i = 0; i < num_input; i++) {
    double dt1 = i > 0 ? 1.0 / (input_times[i] - input_times[i - 1]) : 0.0;
    double dt2 = i < num_input - 1 ? 1.0 / (input_times[i + 1] - input_times[i]) : 0.0;
    if (i > 0 && i < num_input - 1) { dt1 *= 0.5; dt2 *= 0.5; }
    for (int j = 0; j < dim; j++) {
      const size_t row = shift + ni * (dim * i + j);
      if (i - 1 >= 0) point_slope_mapping[row + dim * (i - 1) + j] = -dt1;
      point_slope_mapping[row + dim * i + j] = dt1 - dt2;
      if (i + 1 <= num_input - 1) point_slope_mapping[row + dim * (i + 1) + j] = dt2;
    }
  }
  const size_t no = (size_t)dim * num_output;
  std::fill(output_mapping.begin(), output_mapping.begin() + no * 2 * ni, 0.0);
  int bounds[2];
  double c[4];
  for (int i = 0; i < num_output; i++) {
    FindInterval(bounds, input_times, output_times[i], num_input);
    CubicCoefficients(c, output_times[i], input_times, num_input);
    for (int j = 0; j < dim; j++) {
      const size_t row = 2 * ni * (dim * i + j);
      output_mapping[row + dim * bounds[0] + j] = c[0];
      output_mapping[row + ni + dim * bounds[0] + j] = c[1];
      if (bounds[0] != bounds[1]) {
        output_mapping[row + dim * bounds[1] + j] = c[2];
        output_mapping[row + ni + dim * bounds[1] + j] = c[3];
      }
    }
  }
  for (size_t r = 0; r < no; r++)                                                          // mapping = output_mapping * point_slope_mapping
    for (size_t cc = 0; cc < ni; cc++) {
      double acc = 0.0;
      for (size_t q = 0; q < 2 * ni; q++) acc += output_mapping[r * 2 * ni + q] * point_slope_mapping[q * ni + cc];
      mapping[r * ni + cc] = acc;
    }
}

// ------------------------------------------------------------------ iLQSPlanner (ilqs/planner.cc:33-263)
// The reference solves (A'A) theta = A'u with mju_cholFactor / mju_cholSolve over A = kron(M, I_nu); MuJoCo is not part of this project, so
// the arithmetic is defined here (include/mjpc_hip_planner.h), over the scalar M.
int SplineFitOperator(SplineMapping* mapping, const std::vector<double>& knot_times, int P, const double* action_times, int H1, double* W,
                      std::vector<double>& scratch) {
  mapping->Compute(knot_times, P, action_times, H1);
  const double* M = mapping->Get();                                  // [H1][P]
  scratch.assign((size_t)P * (P + 2), 0.0);
  double *L = scratch.data(), *y = L + (size_t)P * P, *x = y + P;    // G = M'M, overwritten by its lower factor
  for (int i = 0; i < P; i++)
    for (int j = 0; j <= i; j++) {
      double acc = 0.0;
      for (int t = 0; t < H1; t++) acc += M[(size_t)t * P + i] * M[(size_t)t * P + j];
      L[(size_t)i * P + j] = acc;
    }
  for (int i = 0; i < P; i++) {
    for (int j = 0; j < i; j++) {
      double acc = 0.0;
      for (int k = 0; k < j; k++) acc += L[(size_t)i * P + k] * L[(size_t)j * P + k];
      L[(size_t)i * P + j] = (L[(size_t)i * P + j] - acc) / L[(size_t)j * P + j];
    }
    double acc = 0.0;
    for (int k = 0; k < i; k++) acc += L[(size_t)i * P + k] * L[(size_t)i * P + k];
    const double pivot = L[(size_t)i * P + i] - acc;
    if (!(pivot > 0.0) || !std::isfinite(pivot)) return -1;
    L[(size_t)i * P + i] = std::sqrt(pivot);
  }
  for (int t = 0; t < H1; t++) {                                     // column t of W: L L' x = M[t][:]
    for (int i = 0; i < P; i++) {
      double acc = 0.0;
      for (int k = 0; k < i; k++) acc += L[(size_t)i * P + k] * y[k];
      y[i] = (M[(size_t)t * P + i] - acc) / L[(size_t)i * P + i];
    }
    for (int i = P - 1; i >= 0; i--) {
      double acc = 0.0;
      for (int k = i + 1; k < P; k++) acc += L[(size_t)k * P + i] * x[k];
      x[i] = (y[i] - acc) / L[(size_t)i * P + i];
    }
    for (int i = 0; i < P; i++) W[(size_t)i * H1 + t] = x[i];
  }
  return 0;
}

void SplineFitApply(const double* W, int P, int H1, int nu, const double* actions, double* knots) {
  for (int p = 0; p < P; p++)
    for (int j = 0; j < nu; j++) {
      double acc = 0.0;
      for (int t = 0; t < H1; t++) acc += W[(size_t)p * H1 + t] * actions[(size_t)t * nu + j];
      knots[(size_t)p * nu + j] = acc;
    }
}

static std::unique_ptr<SplineMapping> MakeSplineMapping(int representation) {
  std::unique_ptr<SplineMapping> m;
  if (representation == kZeroSpline) m.reset(new ZeroSplineMapping());
  else if (representation == kLinearSpline) m.reset(new LinearSplineMapping());
  else m.reset(new CubicSplineMapping());
  m->Allocate(1);
  return m;
}

int SplineFit(int representation, int P, const double* knot_times, int H1, const double* action_times, int nu, const double* actions,
              double* knots) {
  if (representation < kZeroSpline || representation > kCubicSpline || P < 1 || P > kMaxGradientSplinePoints || H1 < 1 ||
      H1 > kMaxTrajectoryHorizon || nu < 0) return -1;
  std::unique_ptr<SplineMapping> mapping = MakeSplineMapping(representation);
  std::vector<double> W((size_t)P * H1), scratch;
  if (SplineFitOperator(mapping.get(), std::vector<double>(knot_times, knot_times + P), P, action_times, H1, W.data(), scratch) != 0) return -1;
  SplineFitApply(W.data(), P, H1, nu, actions, knots);
  return 0;
}

iLQSPlanner::iLQSPlanner() {
  for (int r = 0; r < 3; r++) mappings[r] = MakeSplineMapping(r);
}

void iLQSPlanner::Initialize(const MjpcHipModel* model, const MjpcHipTask* task, const Numerics& numerics) {
  initialized_ = false;
  // where the reference is undefined (header): refuse instead of producing NaN
  if (numerics.sampling_spline_points < 2) { Fatal("iLQS: sampling_spline_points must be at least 2"); return; }
  if (numerics.sampling_spline_points > kMaxGradientSplinePoints) { Fatal("iLQS: sampling_spline_points exceeds the spline mapping's capacity (25)"); return; }
  if (numerics.sampling_representation == kZeroSpline) { Fatal("iLQS: a zero-order sampling_representation has no spline fit (its normal matrix is singular)"); return; }
  // what the members refuse themselves (their Initialize reports it and leaves them without an engine) leaves this planner inert as well
  const bool sampling_refuses = numerics.sampling_trajectories > numerics.max_samples;
  const bool ilqg_refuses = ilqg.representation < kZeroSpline || ilqg.representation > kCubicSpline || ilqg.num_trajectory < 1 ||
                            ilqg.num_trajectory > kMaxiLQGTrajectory;
  sampling.Initialize(model, task, numerics);
  if (sampling_refuses) return;
  // iLQG's batch is capped at kMaxiLQGTrajectory whatever the sampling batch: its engine needs no more rows than that
  Numerics ilqg_numerics = numerics;
  ilqg_numerics.max_samples = std::min(numerics.max_samples, kMaxiLQGTrajectory);
  ilqg.Initialize(model, task, ilqg_numerics);
  if (ilqg_refuses) return;
  nu_ = model->nu; timestep_ = model->timestep;
  ctrlrange_.assign(model->actuator_ctrlrange, model->actuator_ctrlrange + 2 * nu_);
  initialized_ = true;
}

void iLQSPlanner::Allocate() {
  if (!initialized_) return;
  sampling.Allocate();
  ilqg.Allocate();
  dim_actions = 0; dim_parameters = 0; mapping_representation = -1;
}

void iLQSPlanner::Reset(int horizon, const double* initial_repeated_action) {
  if (!initialized_) return;
  sampling.Reset(horizon, initial_repeated_action);
  ilqg.Reset(horizon, initial_repeated_action);
  active_policy = kSampling; previous_active_policy = kSampling;
  dim_actions = 0; dim_parameters = 0; mapping_representation = -1;
  converted = returned_early = iterated = false;
}

void iLQSPlanner::SetState(const double* s, const double* m, const double* u, double t) {
  if (!initialized_) return;
  sampling.SetState(s, m, u, t);
  ilqg.SetState(s, m, u, t);
}

void iLQSPlanner::SetTask(const MjpcHipTask* task) {
  if (!initialized_) return;
  sampling.SetTask(task);
  ilqg.SetTask(task);
}

bool iLQSPlanner::Convert(int horizon) {   // ilqs/planner.cc:96-169
  auto t0 = std::chrono::steady_clock::now();
  const int P = sampling.policy.num_spline_points, H1 = horizon - 1;
  const int representation = (int)sampling.policy.plan.Interpolation();
  double nominal_time = sampling.time;
  const double time_shift = std::max((horizon - 1) * timestep_ / (P - 1), 1.0e-5);
  spline_times_cache.clear();
  for (int t = 0; t < P; t++) {
    spline_times_cache.push_back(nominal_time);
    nominal_time += time_shift;                           // repeated addition, like the reference
  }
  const Trajectory& nominal = ilqg.candidate.trajectory;
  fit_cache_miss = dim_actions != H1 || dim_parameters != P || mapping_representation != representation;
  if (fit_cache_miss) {
    dim_actions = 0; dim_parameters = 0; mapping_representation = -1;       // nothing valid until the factorisation went through
    inversemapping.resize((size_t)P * H1);
    if (SplineFitOperator(mappings[representation].get(), spline_times_cache, P, nominal.times.data(), H1, inversemapping.data(), fit_scratch_) != 0) {
      fit_compute_time = Micros(t0);
      Fatal("iLQS: spline fit is singular");
      return false;
    }
    dim_actions = H1; dim_parameters = P; mapping_representation = representation;
  }
  spline_parameters_cache.resize((size_t)P * nu_);
  SplineFitApply(inversemapping.data(), P, H1, nu_, nominal.actions.data(), spline_parameters_cache.data());
  for (int t = 0; t < P; t++)
    for (int i = 0; i < nu_; i++) {
      double& v = spline_parameters_cache[(size_t)t * nu_ + i];
      v = std::max(ctrlrange_[2 * i], std::min(ctrlrange_[2 * i + 1], v));   // Clamp
    }
  fit_compute_time = Micros(t0);
  sampling.policy.plan.Clear();
  for (int t = 0; t < P; t++) sampling.policy.plan.AddNode(spline_times_cache[t], spline_parameters_cache.data() + (size_t)t * nu_);
  return true;
}

void iLQSPlanner::OptimizePolicy(int horizon) {   // ilqs/planner.cc:87-214
  if (!initialized_) return;
  converted = returned_early = iterated = false;
  previous_active_policy = active_policy;
  if (previous_active_policy == kiLQG) {
    // sampling optimises a spline: the trajectory-based policy of iLQG (the previous winner) is converted to one first
    if (!ilqg.NominalTrajectory(horizon)) return;
    if (!Convert(horizon)) return;
    converted = true;
  }

  sampling.OptimizePolicy(horizon);

  // winner == 0: there was surely no improvement
  if (sampling.winner > 0 && sampling.returns[sampling.winner] < (previous_active_policy == kSampling ? sampling.returns[0]
                                                                                                      : ilqg.candidate.trajectory.total_return)) {
    if (active_policy == kSampling) ilqg.nominal_compute_time = 0.0;
    ilqg.derivative_compute_time = 0.0;       // model derivatives, cost derivatives and backward pass are one timer here
    ilqg.rollouts_compute_time = 0.0;
    ilqg.policy_update_compute_time = 0.0;
    active_policy = kSampling;
    returned_early = true;
    return;                                   // the best rollout is sampling's
  }
  if (previous_active_policy == kSampling) {
    // candidate_policy[0].trajectory = sampling.trajectory[0]; trajectory_winner is sampling's winner again afterwards
    sampling.FetchCandidateUnranked(0);
    const bool ok = ilqg.SetNominal(sampling.trajectory_winner, horizon);
    if (sampling.winner > 0) sampling.FetchCandidateUnranked(sampling.winner);
    if (!ok) return;
  }

  ilqg.Iteration(horizon);
  iterated = true;

  // adopted nothing (failed backward pass, every rollout failed): the returns below would be an earlier call's
  if (!ilqg.adopted) return;
  if (ilqg.trajectory_winner.total_return < (previous_active_policy == kSampling ? sampling.returns[sampling.winner] : ilqg.returns[0]))
    active_policy = kiLQG;
  // no improvement either way: both policies were updated, active_policy was not
}

void iLQSPlanner::NominalTrajectory(int horizon) {   // ilqs/planner.cc:217-225
  if (!initialized_) return;
  if (active_policy == kSampling) sampling.NominalTrajectory(horizon);
  else ilqg.NominalTrajectory(horizon);
}

int iLQSPlanner::ActionSource(int previous_active, int active, bool use_previous) {   // ilqs/planner.cc:228-253
  if (use_previous) {
    // sampling.OptimizePolicy runs in every call and always updates sampling's policy: its previous one is wanted
    if (previous_active == kSampling) return kSamplingPrevious;
    // the last call returned early: iLQG was not updated, the previous policy is its current one
    if (active == kSampling) return kiLQGCurrent;
    return kiLQGPrevious;
  }
  return active == kSampling ? kSamplingCurrent : kiLQGCurrent;
}

void iLQSPlanner::ActionFromPolicy(double* action, const double* state, double time, bool use_previous) {
  if (!initialized_) return;
  switch (ActionSource(previous_active_policy, active_policy, use_previous)) {
    case kSamplingCurrent: sampling.ActionFromPolicy(action, state, time, false); break;
    case kSamplingPrevious: sampling.ActionFromPolicy(action, state, time, true); break;
    case kiLQGCurrent: ilqg.ActionFromPolicy(action, state, time, false); break;
    default: ilqg.ActionFromPolicy(action, state, time, true); break;
  }
}

const Trajectory* iLQSPlanner::BestTrajectory() {   // ilqs/planner.cc:256-263
  if (!initialized_) return nullptr;
  return active_policy == kSampling ? sampling.BestTrajectory() : ilqg.BestTrajectory();
}

// ------------------------------------------------------------------ GradientPlanner (gradient/planner.cc:40-415)
void GradientPlanner::Refuse(const char* msg) { Fatal(msg); }
GradientPlanner::~GradientPlanner() { if (engine_) mjpc_hip_destroy(engine_); }

void GradientPlanner::Initialize(const MjpcHipModel* model, const MjpcHipTask* task, const Numerics& numerics) {
  numerics_ = numerics;
  ns_ = model->nq + model->nv + model->na; nd_ = 2 * model->nv + model->na; nu_ = model->nu; nr_ = task->num_residual; ntrace_ = task->num_trace;
  nmocap_ = model->nmocap; nuserdata_ = model->nuserdata; timestep_ = model->timestep;
  num_trajectory = numerics.gradient_num_trajectory;
  derivative_skip_ = numerics.derivative_skip;
  if (numerics.gradient_spline_points > kMaxGradientSplinePoints || numerics.gradient_spline_points < 2) {
    char msg[128]; std::snprintf(msg, sizeof(msg), "gradient_spline_points must be 2 .. %d (kMaxGradientSplinePoints).", kMaxGradientSplinePoints);
    Fatal(msg);
    return;
  }
  if (numerics.gradient_representation < kZeroSpline || numerics.gradient_representation > kCubicSpline) { Fatal("Unknown gradient_representation"); return; }
  if (engine_) { mjpc_hip_destroy(engine_); engine_ = nullptr; }
  engine_ = mjpc_hip_create(model, task, std::max(numerics.max_samples, std::max(num_trajectory, 1)), std::max(numerics.max_horizon, 2), numerics.device);
  if (!engine_) { Fatal(mjpc_hip_last_error()); return; }
  const int Hm = numerics.max_horizon;
  for (GradientPolicy* p : {&policy, &previous_policy, &nominal_policy}) p->Allocate(model, numerics, std::max(Hm, kMaxGradientSplinePoints));
  mappings[kZeroSpline].reset(new ZeroSplineMapping()); mappings[kLinearSpline].reset(new LinearSplineMapping()); mappings[kCubicSpline].reset(new CubicSplineMapping());
}

void GradientPlanner::Allocate() {
  if (!engine_) return;
  const size_t Hm = (size_t)numerics_.max_horizon;
  state.assign(ns_, 0.0); mocap.assign(7 * nmocap_, 0.0); userdata.assign(nuserdata_, 0.0);
  for (Trajectory* tr : {&trajectory_nominal, &trajectory_winner}) {
    tr->dim_state = ns_; tr->dim_action = nu_; tr->dim_residual = nr_; tr->dim_trace = 3 * ntrace_;
    tr->states.assign(Hm * ns_, 0.0); tr->actions.assign(Hm * nu_, 0.0); tr->times.assign(Hm, 0.0); tr->residual.assign(Hm * nr_, 0.0);
    tr->costs.assign(Hm, 0.0); tr->trace.assign(Hm * 3 * std::max(ntrace_, 1), 0.0);
  }
  model_derivative.Allocate(nd_, nu_, nr_, (int)Hm, ns_);
  cost_derivative.Allocate(nd_, nu_, nr_, (int)Hm);
  gradient.Allocate(nd_, nu_, (int)Hm);
  for (auto& m : mappings) m->Allocate(nu_);
  parameters_scratch_.assign((size_t)nu_ * kMaxGradientSplinePoints, 0.0); times_scratch_.assign(kMaxGradientSplinePoints, 0.0);
  winner = -1;
}

void GradientPlanner::Reset(int horizon, const double* initial_repeated_action) {
  std::fill(state.begin(), state.end(), 0.0); std::fill(mocap.begin(), mocap.end(), 0.0); std::fill(userdata.begin(), userdata.end(), 0.0);
  time = 0.0;
  const int h = horizon > 0 ? std::min(horizon, numerics_.max_horizon) : numerics_.max_horizon;
  model_derivative.Reset(nd_, nu_, nr_, h); cost_derivative.Reset(nd_, nu_, nr_, h); gradient.Reset(nd_, nu_, h);
  for (GradientPolicy* p : {&policy, &previous_policy, &nominal_policy}) p->Reset(std::max(h, kMaxGradientSplinePoints), initial_repeated_action);
  action_step = 0.0; expected = 0.0; improvement = 0.0; surprise = 0.0;
  winner = -1; failed = false;
  derivative_skip_ = numerics_.derivative_skip;
}

void GradientPlanner::SetState(const double* s, const double* m, const double* u, double t) {
  std::copy(s, s + ns_, state.begin());
  if (m) std::copy(m, m + 7 * nmocap_, mocap.begin());
  if (u) std::copy(u, u + nuserdata_, userdata.begin());
  time = t;
}

void GradientPlanner::SetTask(const MjpcHipTask* task) { if (mjpc_hip_set_task(engine_, task) != 0) Fatal(mjpc_hip_last_error()); }

void GradientPlanner::ActionFromPolicy(double* action, const double* s, double t, bool use_previous) {
  const std::shared_lock<std::shared_mutex> lock(mtx_);
  (use_previous ? previous_policy : policy).Action(action, s, t);
}

void GradientPlanner::ResamplePolicy(int horizon) {   // planner.cc:330-358
  GradientPolicy& cp = nominal_policy;
  const int P = cp.num_spline_points;
  double nominal_time = time;
  const double time_shift = std::max((horizon - 1) * timestep_ / (P - 1), 1.0e-5);
  for (int t = 0; t < P; t++) {
    times_scratch_[t] = nominal_time;
    cp.Action(parameters_scratch_.data() + (size_t)t * nu_, nullptr, nominal_time);
    nominal_time += time_shift;
  }
  std::copy(parameters_scratch_.begin(), parameters_scratch_.begin() + (size_t)P * nu_, cp.parameters.begin());
  const double t0 = times_scratch_[0];
  for (int t = 0; t < P; t++) cp.times[t] = t0 + t * time_shift;                         // LinearRange
}

bool GradientPlanner::Rollout(const double* knots, int n, int horizon) {
  returns.assign(n, 0.0); failures.assign(n, 0);
  MjpcHipPlanInput in = MakePlanInput(state.data(), mocap.data(), userdata.data(), time, nominal_policy.times.data(), knots, nominal_policy.num_spline_points,
                                      nominal_policy.representation, n, horizon);
  in.candidate_knots = knots;
  MjpcHipPlanOutput out;
  std::memset(&out, 0, sizeof(out));
  out.returns = returns.data(); out.failure = failures.data();
  const int rc = mjpc_hip_plan(engine_, &in, &out);
  if (rc != 0 && rc != -3) { Fatal(mjpc_hip_last_error()); return false; }               // -3: no finite return; returns[] are valid
  return true;
}

// trajectory `index` of the last plan into tr
static bool FetchCandidate(MjpcHipEngine* engine, int index, int horizon, double total_return, int failure, Trajectory& tr) {
  MjpcHipPlanOutput out;
  std::memset(&out, 0, sizeof(out));
  out.states = tr.states.data(); out.actions = tr.actions.data(); out.times = tr.times.data();
  out.residual = tr.residual.data(); out.costs = tr.costs.data(); out.trace = tr.trace.data();
  if (mjpc_hip_get_candidate(engine, index, &out) != 0) { Fatal(mjpc_hip_last_error()); return false; }
  tr.horizon = horizon; tr.total_return = total_return; tr.failure = failure != 0;
  return true;
}

void GradientPlanner::NominalTrajectory(int horizon) {
  if (!Rollout(nominal_policy.parameters.data(), 1, horizon)) return;
  FetchCandidate(engine_, 0, horizon, returns[0], failures[0], trajectory_nominal);
}

void GradientPlanner::OptimizePolicy(int horizon) {
  using clock = std::chrono::steady_clock;
  auto us = [](clock::time_point t0) { return std::chrono::duration<double, std::micro>(clock::now() - t0).count(); };
  if (!engine_) return;
  if (horizon < 2 || horizon > numerics_.max_horizon) { Fatal("GradientPlanner: horizon out of range (2 .. max_horizon)"); return; }
  nominal_compute_time = derivative_compute_time = gradient_compute_time = rollouts_compute_time = policy_update_compute_time = 0.0;
  failed = false;
  num_trajectory = std::max(1, std::min(num_trajectory, numerics_.max_samples));
  const int N = num_trajectory, P = policy.num_spline_points, PN = P * nu_;

  // ----- nominal rollout -----
  auto t0 = clock::now();
  policy.num_parameters = PN;
  { const std::shared_lock<std::shared_mutex> lock(mtx_); nominal_policy.CopyFrom(policy, P); }
  ResamplePolicy(horizon);
  NominalTrajectory(horizon);
  const double c_prev = trajectory_nominal.total_return;
  nominal_compute_time = us(t0);

  double c_best = c_prev;
  cand_knots_.assign((size_t)N * PN, 0.0);
  linesearch_steps.assign(N, 0.0);
  std::vector<int> fail(horizon, 0);
  for (int it = 0; it < settings.max_rollout; it++) {
    // ----- derivatives and gradient of the nominal trajectory -----
    t0 = clock::now();
    const Trajectory& tr = trajectory_nominal;
    bool ok;
    if (derivative_skip_ <= 0) {
      ok = mjpc_hip_trajectory_gradient(engine_, horizon, tr.states.data(), tr.actions.data(), tr.times.data(), tr.residual.data(), mocap.data(), userdata.data(),
                                        settings.fd_tolerance, settings.fd_mode, nominal_policy.k.data(), gradient.Vx.data(), gradient.Qx.data(),
                                        gradient.Qu.data(), gradient.dV, fail.data()) == 0;
    } else {
      ok = model_derivative.Compute(engine_, tr.states.data(), tr.actions.data(), tr.times.data(), horizon, settings.fd_tolerance, settings.fd_mode,
                                    derivative_skip_, mocap.data(), userdata.data()) &&
           cost_derivative.Compute(engine_, tr.residual.data(), model_derivative.C.data(), model_derivative.D.data(), nd_, nu_, nr_, horizon, false);
      if (ok) {
        std::copy(model_derivative.failure.begin(), model_derivative.failure.begin() + horizon, fail.begin());
        ok = gradient.Compute(nominal_policy.k.data(), &model_derivative, &cost_derivative, nd_, nu_, horizon) == 0;
      }
    }
    derivative_compute_time += us(t0);
    if (!ok) { Fatal(mjpc_hip_last_error()); failed = true; return; }
    for (int t = 0; t < horizon; t++) if (fail[t]) { failed = true; return; }             // like gd_status != 0: the policy stays as it was

    // ----- total derivative: parameter_update = M' k -----
    t0 = clock::now();
    SplineMapping& map = *mappings[policy.representation];
    map.Compute(nominal_policy.times, P, tr.times.data(), horizon - 1);
    const int rows = nu_ * (horizon - 1);
    for (int c = 0; c < PN; c++) {
      double acc = 0.0;
      for (int r = 0; r < rows; r++) acc += map.mapping[(size_t)r * PN + c] * nominal_policy.k[r];
      nominal_policy.parameter_update[c] = acc;
    }
    gradient_compute_time += us(t0);

    // ----- line search: one plan of N explicit candidates -----
    t0 = clock::now();
    if (N > 1) {     // LogScale as the reference spells it: exp(log(min) + i * step), no pinned first value
      const double lo = std::log(settings.min_linesearch_step), step = (std::log(1.0) - lo) / std::max(N - 2, 1);
      for (int i = 0; i < N - 1; i++) linesearch_steps[i] = std::exp(lo + i * step);
    }
    linesearch_steps[N - 1] = 0.0;
    for (int i = 0; i < N; i++)
      for (int c = 0; c < PN; c++) cand_knots_[(size_t)i * PN + c] = nominal_policy.parameters[c] + nominal_policy.parameter_update[c] * linesearch_steps[i];
    if (!Rollout(cand_knots_.data(), N, horizon)) return;
    winner = N - 1;
    for (int j = N - 1; j >= 0; j--)
      if (returns[j] < c_best) { c_best = returns[j]; winner = j; }
    std::copy(cand_knots_.begin() + (size_t)winner * PN, cand_knots_.begin() + (size_t)(winner + 1) * PN, nominal_policy.parameters.begin());
    if (!FetchCandidate(engine_, winner, horizon, returns[winner], failures[winner], trajectory_nominal)) return;
    action_step = linesearch_steps[winner];
    expected = -action_step * gradient.dV[0] - 1.0e-16;
    improvement = c_prev - c_best;
    surprise = std::min(std::max(0.0, improvement / expected), 2.0);
    rollouts_compute_time += us(t0);
  }

  // ----- update the nominal policy -----
  t0 = clock::now();
  if (settings.max_rollout < 1) { winner = -1; return; }
  if (c_best >= c_prev) winner = N - 1;
  trajectory_winner = trajectory_nominal;               // (candidate N - 1 is the nominal itself: step 0)
  {
    const std::unique_lock<std::shared_mutex> lock(mtx_);
    previous_policy.CopyFrom(policy, P);
    policy.CopyParametersFrom(nominal_policy.parameters, nominal_policy.times);
  }
  policy_update_compute_time = us(t0);
}

// ------------------------------------------------------------------ Estimators: Kalman, Unscented (mjpc/estimators/)
// The algebra by the summation rule of this file: ascending contraction index from 0.0, a rounded product and a rounded add per step.
namespace {
void Symmetrize(double* P, int n) {            // mju_symmetrize
  for (int i = 0; i < n; i++)
    for (int j = i + 1; j < n; j++) {
      const double v = 0.5 * (P[(size_t)i * n + j] + P[(size_t)j * n + i]);
      P[(size_t)i * n + j] = v; P[(size_t)j * n + i] = v;
    }
}
// res [r1][r2] = A B', A [r1][c], B [r2][c]
void MulMatMatT(double* res, const double* A, const double* B, int r1, int c, int r2) {
  for (int i = 0; i < r1; i++)
    for (int j = 0; j < r2; j++) {
      double s = 0.0;
      for (int k = 0; k < c; k++) s += A[(size_t)i * c + k] * B[(size_t)j * c + k];
      res[(size_t)i * r2 + j] = s;
    }
}
bool CholFactorFull(double* L, const double* H, int n) {
  std::vector<int> identity(n);
  for (int i = 0; i < n; i++) identity[i] = i;
  return n == 0 || CholFactorSub(L, H, n, identity.data(), n);
}
// ukf_sincos / ukf_quatintegrate of csrc/estimator.h, operation for operation (this file is compiled without contraction): the same bits
// as the sigma-point kernel's and the emulation's
void SinCosRn(double x, double* sn, double* cs) {
  if (!(std::fabs(x) < 64.0)) { *sn = std::sin(x); *cs = std::cos(x); return; }
  const double k = std::rint(x * 0.63661977236758134308);
  const double r = (x + -(k * 1.57079632673412561417e+00)) + -(k * 6.07710050650619224932e-11);
  const double z = r * r;
  double ps = 1.58969099521155010221e-10, pc = -1.13596475577881948265e-11;
  const double S[5] = {-2.50507602534068634195e-08, 2.75573137070700676789e-06, -1.98412698298579493134e-04, 8.33333333332248946124e-03, -1.66666666666666324348e-01};
  const double C[5] = {2.08757232129817482790e-09, -2.75573143513906633035e-07, 2.48015872894767294178e-05, -1.38888888888741095749e-03, 4.16666666666666019037e-02};
  for (int i = 0; i < 5; i++) { ps = S[i] + z * ps; pc = C[i] + z * pc; }
  const double s = r + (r * z) * ps;
  const double c = (1.0 + -(0.5 * z)) + (z * z) * pc;
  const int q = ((int)k) & 3;
  const double s1 = (q & 1) ? c : s, c1 = (q & 1) ? s : c;
  *sn = (q & 2) ? -s1 : s1;
  *cs = ((q + 1) & 2) ? -c1 : c1;
}
void Normalize4(double* q) {
  const double n2 = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3];
  const double n = std::sqrt(n2);
  if (n < 1e-15) { q[0] = 1; q[1] = 0; q[2] = 0; q[3] = 0; }
  else if (std::fabs(n - 1) > 1e-15) { q[0] = q[0] / n; q[1] = q[1] / n; q[2] = q[2] / n; q[3] = q[3] / n; }
}
void QuatIntegrate(double* q, const double* vel, double scale) {
  double ax[3] = {vel[0], vel[1], vel[2]};
  const double n = std::sqrt((ax[0] * ax[0] + ax[1] * ax[1]) + ax[2] * ax[2]);
  if (n < 1e-15) { ax[0] = 1; ax[1] = 0; ax[2] = 0; }
  else { ax[0] = ax[0] / n; ax[1] = ax[1] / n; ax[2] = ax[2] / n; }
  const double angle = scale * n;
  double b[4] = {1, 0, 0, 0};
  if (angle != 0) {
    double sn, cs;
    SinCosRn(angle * 0.5, &sn, &cs);
    b[0] = cs; b[1] = ax[0] * sn; b[2] = ax[1] * sn; b[3] = ax[2] * sn;
  }
  Normalize4(q);
  const double a[4] = {q[0], q[1], q[2], q[3]};
  q[0] = ((a[0] * b[0] + -(a[1] * b[1])) + -(a[2] * b[2])) + -(a[3] * b[3]);
  q[1] = ((a[0] * b[1] + a[1] * b[0]) + a[2] * b[3]) + -(a[3] * b[2]);
  q[2] = ((a[0] * b[2] + -(a[1] * b[3])) + a[2] * b[0]) + a[3] * b[1];
  q[3] = ((a[0] * b[3] + a[1] * b[2]) + -(a[2] * b[1])) + a[3] * b[0];
  Normalize4(q);
}
}  // namespace

bool CovarianceFactor(int n, const double* P, double* L) {
  std::vector<double> tmp((size_t)n * n, 0.0);
  if (!CholFactorFull(tmp.data(), P, n)) return false;
  std::copy(tmp.begin(), tmp.end(), L);
  return true;
}

int KalmanGain(int nd, int ns, const double* P, const double* C, const double* R, double* PCt, double* factor, double* gain) {
  std::vector<double> pct((size_t)nd * ns), S((size_t)ns * ns), F((size_t)ns * ns, 0.0);
  MulMatMatT(pct.data(), P, C, nd, nd, ns);                 // P C'
  MulMatMat(S.data(), C, pct.data(), ns, nd, ns);           // C (P C')
  for (int i = 0; i < ns; i++) S[(size_t)i * ns + i] += R[i];
  if (!CholFactorFull(F.data(), S.data(), ns)) return kEstimatorSensorRank;
  std::copy(pct.begin(), pct.end(), PCt);
  std::copy(F.begin(), F.end(), factor);
  for (int i = 0; i < nd; i++) CholSolveSub(gain + (size_t)i * ns, F.data(), ns, PCt + (size_t)i * ns);     // column by column of the gain's transpose
  return kEstimatorOk;
}

void KalmanCorrect(int nd, int ns, const double* PCt, const double* factor, const double* gain, const double* sensor_error, double* correction,
                   double* P) {
  std::vector<double> y(ns), D((size_t)nd * nd);
  CholSolveSub(y.data(), factor, ns, sensor_error);
  MulMatMat(correction, PCt, y.data(), nd, ns, 1);
  MulMatMatT(D.data(), PCt, gain, nd, ns, nd);
  for (size_t e = 0; e < (size_t)nd * nd; e++) P[e] = P[e] - D[e];
  Symmetrize(P, nd);
}

void CovariancePredict(int nd, const double* A, const double* Q, double* P) {
  std::vector<double> PAt((size_t)nd * nd), N((size_t)nd * nd);
  MulMatMatT(PAt.data(), P, A, nd, nd, nd);
  MulMatMat(N.data(), A, PAt.data(), nd, nd, nd);
  for (int i = 0; i < nd; i++) N[(size_t)i * nd + i] += Q[i];
  std::copy(N.begin(), N.end(), P);
  Symmetrize(P, nd);
}

int UnscentedCorrect(int nd, int ns, const double* cov_ss, const double* cov_sy, const double* cov_yy, const double* sensor_error,
                     double* correction, double* P) {
  std::vector<double> F((size_t)ns * ns, 0.0), y(ns), G((size_t)nd * ns), D((size_t)nd * nd);
  if (!CholFactorFull(F.data(), cov_yy, ns)) return kEstimatorSensorRank;
  CholSolveSub(y.data(), F.data(), ns, sensor_error);
  MulMatMat(correction, cov_sy, y.data(), nd, ns, 1);
  for (int i = 0; i < nd; i++) CholSolveSub(G.data() + (size_t)i * ns, F.data(), ns, cov_sy + (size_t)i * ns);
  MulMatMatT(D.data(), cov_sy, G.data(), nd, ns, nd);
  for (size_t e = 0; e < (size_t)nd * nd; e++) P[e] = cov_ss[e] - D[e];
  Symmetrize(P, nd);
  return kEstimatorOk;
}

int Estimator::Initialize(MjpcHipEngine* engine, const MjpcHipModel* model, const MjpcHipTask* task, int sensor_first_row, int num_sensor,
                          const EstimatorSettings& s) {
  engine_ = engine; settings = s;
  nq = model->nq; nv = model->nv; na = model->na; nu = model->nu; nr = task->num_residual; nd = 2 * nv + na;
  ns = num_sensor; first = sensor_first_row; timestep = model->timestep;
  if (!engine || ns < 1 || first < 0 || first + ns > nr) return -1;
  jnt_type_.assign(model->jnt_type, model->jnt_type + model->njnt);
  jnt_qposadr_.assign(model->jnt_qposadr, model->jnt_qposadr + model->njnt);
  jnt_dofadr_.assign(model->jnt_dofadr, model->jnt_dofadr + model->njnt);
  state.assign(nq + nv + na, 0.0); covariance.assign((size_t)nd * nd, 0.0); noise_process.assign(nd, 0.0); noise_sensor.assign(ns, 0.0);
  mocap_.assign(7 * (size_t)model->nmocap, 0.0); userdata_.assign(model->nuserdata, 0.0); ctrl_.assign(nu, 0.0);
  for (int i = 0; i < model->nmocap; i++) mocap_[7 * i + 3] = 1.0;
  Reset(state.data(), 0.0);
  return 0;
}

void Estimator::Reset(const double* st, double t) {
  if (st != state.data()) std::copy(st, st + nq + nv + na, state.begin());
  time = t;
  std::fill(covariance.begin(), covariance.end(), 0.0);
  for (int i = 0; i < nd; i++) covariance[(size_t)i * nd + i] = settings.covariance_initial_scale;
  std::fill(noise_process.begin(), noise_process.end(), settings.process_noise_scale);
  std::fill(noise_sensor.begin(), noise_sensor.end(), settings.sensor_noise_scale);
  last_failure = 0;
}

void Estimator::SetShared(const double* mocap, const double* userdata) {
  if (mocap) std::copy(mocap, mocap + mocap_.size(), mocap_.begin());
  if (userdata) std::copy(userdata, userdata + userdata_.size(), userdata_.begin());
}

void Estimator::IntegrateState(double* x, const double* c) const {
  for (size_t j = 0; j < jnt_type_.size(); j++) {
    const int qa = jnt_qposadr_[j], da = jnt_dofadr_[j];
    if (jnt_type_[j] == 0) { for (int k = 0; k < 3; k++) x[qa + k] = x[qa + k] + c[da + k]; QuatIntegrate(x + qa + 3, c + da + 3, 1.0); }
    else if (jnt_type_[j] == 1) QuatIntegrate(x + qa, c + da, 1.0);
    else x[qa] = x[qa] + c[da];
  }
  for (int i = 0; i < nv + na; i++) x[nq + i] = x[nq + i] + c[nv + i];
}

int Kalman::UpdateMeasurement(const double* ctrl, const double* sensor) {
  next_.resize(state.size()); residual_.resize(nr); A_.resize((size_t)nd * nd); C_.resize((size_t)nr * nd);
  PCt_.resize((size_t)nd * ns); factor_.resize((size_t)ns * ns); gain_.resize((size_t)nd * ns); error_.resize(ns); correction_.resize(nd);
  if (nu) std::copy(ctrl, ctrl + nu, ctrl_.begin());
  if (mjpc_hip_linearize_step(engine_, state.data(), ctrl_.data(), time, mocap_.data(), userdata_.data(), settings.epsilon, settings.flg_centered ? 1 : 0,
                              nullptr, residual_.data(), nullptr, C_.data(), &last_failure) != 0) return kEstimatorEngineError;
  if (last_failure) return kEstimatorStepFlagged;
  const double* C = C_.data() + (size_t)first * nd;
  const int rc = KalmanGain(nd, ns, covariance.data(), C, noise_sensor.data(), PCt_.data(), factor_.data(), gain_.data());
  if (rc != kEstimatorOk) return rc;
  for (int i = 0; i < ns; i++) error_[i] = sensor[i] - residual_[first + i];
  KalmanCorrect(nd, ns, PCt_.data(), factor_.data(), gain_.data(), error_.data(), correction_.data(), covariance.data());
  IntegrateState(state.data(), correction_.data());
  return kEstimatorOk;
}

int Kalman::UpdatePrediction() {
  next_.resize(state.size()); A_.resize((size_t)nd * nd);
  if (mjpc_hip_linearize_step(engine_, state.data(), ctrl_.data(), time, mocap_.data(), userdata_.data(), settings.epsilon, settings.flg_centered ? 1 : 0,
                              next_.data(), nullptr, A_.data(), nullptr, &last_failure) != 0) return kEstimatorEngineError;
  if (last_failure) return kEstimatorStepFlagged;
  state = next_;
  CovariancePredict(nd, A_.data(), noise_process.data(), covariance.data());
  time += timestep;
  return kEstimatorOk;
}

int Kalman::Update(const double* ctrl, const double* sensor) {
  const std::vector<double> state0 = state, covariance0 = covariance;
  int rc = UpdateMeasurement(ctrl, sensor);
  if (rc != kEstimatorOk) return rc;
  rc = UpdatePrediction();
  if (rc != kEstimatorOk) { state = state0; covariance = covariance0; }
  return rc;
}

int Unscented::Initialize(MjpcHipEngine* engine, const MjpcHipModel* model, const MjpcHipTask* task, int sensor_first_row, int num_sensor,
                          const EstimatorSettings& s) {
  const int rc = Estimator::Initialize(engine, model, task, sensor_first_row, num_sensor, s);
  const double lambda = nd * (s.alpha * s.alpha - 1.0);
  sigma_step = std::sqrt(nd + lambda);
  weight_mean0 = lambda / (nd + lambda);
  weight_covariance0 = weight_mean0 + 1.0 - s.alpha * s.alpha + s.beta;
  weight_sigma = 1.0 / (2.0 * (nd + lambda));
  return rc;
}

int Unscented::Update(const double* ctrl, const double* sensor) {
  const size_t ds = state.size(), n = nd, m = ns;
  factor_.resize(n * n); state_mean_.resize(ds); sensor_mean_.resize(m); cov_ss_.resize(n * n); cov_sy_.resize(n * m); cov_yy_.resize(m * m);
  error_.resize(m); correction_.resize(n); P_.resize(n * n); sigma_next.resize((2 * n + 1) * ds);
  if (nu) std::copy(ctrl, ctrl + nu, ctrl_.begin());
  if (!CovarianceFactor(nd, covariance.data(), factor_.data())) return kEstimatorCovarianceRank;
  const double w[3] = {weight_mean0, weight_covariance0, weight_sigma};
  if (mjpc_hip_unscented_moments(engine_, state.data(), factor_.data(), sigma_step, w, ctrl_.data(), time, mocap_.data(), userdata_.data(),
                                 noise_process.data(), noise_sensor.data(), first, ns, state_mean_.data(), sensor_mean_.data(), cov_ss_.data(),
                                 cov_sy_.data(), cov_yy_.data(), sigma_next.data(), &last_failure) != 0) return kEstimatorEngineError;
  if (last_failure) return kEstimatorStepFlagged;
  for (int i = 0; i < ns; i++) error_[i] = sensor[i] - sensor_mean_[i];
  const int rc = UnscentedCorrect(nd, ns, cov_ss_.data(), cov_sy_.data(), cov_yy_.data(), error_.data(), correction_.data(), P_.data());
  if (rc != kEstimatorOk) return rc;
  state = state_mean_;
  IntegrateState(state.data(), correction_.data());
  covariance = P_;
  time += timestep;
  return kEstimatorOk;
}

}  // namespace mjpc_hip

// ====================================================================== flat C wrapper (tests / ctypes)
using mjpc_hip::SamplingPlanner;
using mjpc_hip::TimeSpline;

// a trajectory for the flat C view: returns its horizon (0 if there is none); copies the arrays that are non-null
static int CopyTrajectory(const mjpc_hip::Trajectory* t, double* states, double* actions, double* times, double* residual, double* costs,
                          double* trace, double* total_return, int* failure) {
  if (!t) return 0;
  size_t H = (size_t)t->horizon;
  if (states) std::copy(t->states.begin(), t->states.begin() + H * t->dim_state, states);
  if (actions) std::copy(t->actions.begin(), t->actions.begin() + H * t->dim_action, actions);
  if (times) std::copy(t->times.begin(), t->times.begin() + H, times);
  if (residual) std::copy(t->residual.begin(), t->residual.begin() + H * t->dim_residual, residual);
  if (costs) std::copy(t->costs.begin(), t->costs.begin() + H, costs);
  if (trace) std::copy(t->trace.begin(), t->trace.begin() + H * t->dim_trace, trace);
  if (total_return) *total_return = t->total_return;
  if (failure) *failure = t->failure ? 1 : 0;
  return t->horizon;
}

extern "C" {

void mjpc_planner_set_error_handler(void (*h)(const char*)) { mjpc_hip::g_error_handler = h; }

// ---- TimeSpline (so that the reference's spline goldens can be run against the C++ class)
void* mjpc_spline_create(int dim, int interpolation) { return new TimeSpline(dim, (mjpc_hip::SplineInterpolation)interpolation); }
void mjpc_spline_destroy(void* s) { delete (TimeSpline*)s; }
int mjpc_spline_size(void* s) { return (int)((TimeSpline*)s)->Size(); }
void mjpc_spline_add_node(void* s, double time, const double* values) { ((TimeSpline*)s)->AddNode(time, values); }
void mjpc_spline_sample(void* s, double time, double* out) { ((TimeSpline*)s)->Sample(time, out); }
int mjpc_spline_discard_before(void* s, double time) { return ((TimeSpline*)s)->DiscardBefore(time); }
void mjpc_spline_clear(void* s) { ((TimeSpline*)s)->Clear(); }
void mjpc_spline_set_interpolation(void* s, int i) { ((TimeSpline*)s)->SetInterpolation((mjpc_hip::SplineInterpolation)i); }

// ---- SamplingPlanner
void* mjpc_planner_create(const MjpcHipModel* model, const MjpcHipTask* task, const double* exploration, int trajectories,
                          int representation, int sliding_plan, int spline_points, int max_samples, int max_horizon, int device) {
  auto* p = new SamplingPlanner();
  mjpc_hip::Numerics n;
  n.sampling_exploration[0] = exploration[0]; n.sampling_exploration[1] = exploration[1];
  n.sampling_trajectories = trajectories; n.sampling_representation = representation; n.sampling_sliding_plan = sliding_plan;
  n.sampling_spline_points = spline_points; n.max_samples = max_samples; n.max_horizon = max_horizon; n.device = device;
  p->Initialize(model, task, n);
  p->Allocate();
  return p;
}
// the same planner with its candidate batch sharded over n_devices GPUs (devices[k]: HIP ordinals, repeats allowed)
void* mjpc_planner_create_sharded(const MjpcHipModel* model, const MjpcHipTask* task, const double* exploration, int trajectories,
                                  int representation, int sliding_plan, int spline_points, int max_samples, int max_horizon,
                                  int n_devices, const int* devices) {
  auto* p = new SamplingPlanner();
  mjpc_hip::Numerics n;
  n.sampling_exploration[0] = exploration[0]; n.sampling_exploration[1] = exploration[1];
  n.sampling_trajectories = trajectories; n.sampling_representation = representation; n.sampling_sliding_plan = sliding_plan;
  n.sampling_spline_points = spline_points; n.max_samples = max_samples; n.max_horizon = max_horizon;
  n.n_devices = n_devices; n.device = (devices && n_devices > 0) ? devices[0] : 0;
  if (devices) n.devices.assign(devices, devices + n_devices);
  p->Initialize(model, task, n);
  p->Allocate();
  return p;
}
void mjpc_planner_destroy(void* p) { delete (SamplingPlanner*)p; }
void mjpc_planner_reset(void* p, int horizon, const double* initial_repeated_action) { ((SamplingPlanner*)p)->Reset(horizon, initial_repeated_action); }
void mjpc_planner_set_state(void* p, const double* s, const double* m, const double* u, double t) { ((SamplingPlanner*)p)->SetState(s, m, u, t); }
void mjpc_planner_set_task(void* p, const MjpcHipTask* task) { ((SamplingPlanner*)p)->SetTask(task); }
void mjpc_planner_timings(void* p, double* a, double* b, double* c) { auto* q = (SamplingPlanner*)p; *a = q->noise_compute_time; *b = q->rollouts_compute_time; *c = q->policy_update_compute_time; }
void mjpc_planner_optimize_policy(void* p, int horizon) { ((SamplingPlanner*)p)->OptimizePolicy(horizon); }
void mjpc_planner_nominal_trajectory(void* p, int horizon) { ((SamplingPlanner*)p)->NominalTrajectory(horizon); }
void mjpc_planner_action_from_policy(void* p, double* action, double time, int use_previous) { ((SamplingPlanner*)p)->ActionFromPolicy(action, nullptr, time, use_previous != 0); }
int mjpc_planner_optimize_policy_candidates(void* p, int ncandidates, int horizon) { auto* q = (SamplingPlanner*)p; q->UpdateNominalPolicy(horizon); return q->OptimizePolicyCandidates(ncandidates, horizon); }
double mjpc_planner_candidate_score(void* p, int candidate) { return ((SamplingPlanner*)p)->CandidateScore(candidate); }
void mjpc_planner_action_from_candidate_policy(void* p, double* action, int candidate, double time) { ((SamplingPlanner*)p)->ActionFromCandidatePolicy(action, candidate, nullptr, time); }
void mjpc_planner_copy_candidate_to_policy(void* p, int candidate) { ((SamplingPlanner*)p)->CopyCandidateToPolicy(candidate); }
int mjpc_planner_winner(void* p) { return ((SamplingPlanner*)p)->winner; }
double mjpc_planner_improvement(void* p) { return ((SamplingPlanner*)p)->improvement; }
int mjpc_planner_num_parameters(void* p) { return ((SamplingPlanner*)p)->NumParameters(); }
void mjpc_planner_set_seed(void* p, unsigned long long seed, unsigned long long plan_iter) { auto* q = (SamplingPlanner*)p; q->seed = seed; q->plan_iter = plan_iter; }
void mjpc_planner_set_num_trajectory(void* p, int n) { ((SamplingPlanner*)p)->num_trajectory_ = n; }
void mjpc_planner_set_noise(void* p, const double* eps, const int* sel) { auto* q = (SamplingPlanner*)p; q->injected_noise_eps = eps; q->injected_noise_sel = sel; }
void mjpc_planner_returns(void* p, double* out, int n) { auto* q = (SamplingPlanner*)p; std::copy(q->returns.begin(), q->returns.begin() + n, out); }
int mjpc_planner_policy(void* p, int which, double* times, double* values) {
  auto* q = (SamplingPlanner*)p;
  return mjpc_hip::CopyKnots(which ? q->previous_policy : q->policy, times, values);
}
int mjpc_planner_best_trajectory(void* p, double* states, double* actions, double* times, double* residual, double* costs,
                                 double* trace, double* total_return, int* failure) {
  return CopyTrajectory(((SamplingPlanner*)p)->BestTrajectory(), states, actions, times, residual, costs, trace, total_return, failure);
}

// ---- CrossEntropyPlanner
void* mjpc_cem_create(const MjpcHipModel* model, const MjpcHipTask* task, double std_initial, double std_min, int trajectories,
                      int n_elite, int representation, int spline_points, int max_samples, int max_horizon, int device) {
  auto* p = new mjpc_hip::CrossEntropyPlanner();
  mjpc_hip::Numerics n;
  n.sampling_exploration[0] = std_initial; n.std_min = std_min; n.sampling_trajectories = trajectories; n.n_elite = n_elite;
  n.sampling_representation = representation; n.sampling_spline_points = spline_points; n.max_samples = max_samples;
  n.max_horizon = max_horizon; n.device = device;
  p->Initialize(model, task, n);
  p->Allocate();
  return p;
}
void mjpc_cem_destroy(void* p) { delete (mjpc_hip::CrossEntropyPlanner*)p; }
void mjpc_cem_reset(void* p, int horizon, const double* a) { ((mjpc_hip::CrossEntropyPlanner*)p)->Reset(horizon, a); }
void mjpc_cem_set_state(void* p, const double* s, const double* m, const double* u, double t) { ((mjpc_hip::CrossEntropyPlanner*)p)->SetState(s, m, u, t); }
void mjpc_cem_set_seed(void* p, unsigned long long seed, unsigned long long it) { auto* q = (mjpc_hip::CrossEntropyPlanner*)p; q->seed = seed; q->plan_iter = it; }
void mjpc_cem_set_noise(void* p, const double* eps) { ((mjpc_hip::CrossEntropyPlanner*)p)->injected_noise_eps = eps; }
void mjpc_cem_optimize_policy(void* p, int horizon) { ((mjpc_hip::CrossEntropyPlanner*)p)->OptimizePolicy(horizon); }
void mjpc_cem_nominal_trajectory(void* p, int horizon) { ((mjpc_hip::CrossEntropyPlanner*)p)->NominalTrajectory(horizon); }
void mjpc_cem_action_from_policy(void* p, double* a, double t, int prev) { ((mjpc_hip::CrossEntropyPlanner*)p)->ActionFromPolicy(a, nullptr, t, prev != 0); }
double mjpc_cem_improvement(void* p) { return ((mjpc_hip::CrossEntropyPlanner*)p)->improvement; }
void mjpc_cem_returns(void* p, double* out, int n) { auto* q = (mjpc_hip::CrossEntropyPlanner*)p; std::copy(q->returns.begin(), q->returns.begin() + n, out); }
void mjpc_cem_variance(void* p, double* out, int n) { auto* q = (mjpc_hip::CrossEntropyPlanner*)p; std::copy(q->variance.begin(), q->variance.begin() + n, out); }
int mjpc_cem_policy(void* p, double* times, double* values) { return mjpc_hip::CopyKnots(((mjpc_hip::CrossEntropyPlanner*)p)->policy, times, values); }
int mjpc_cem_best_trajectory(void* p, double* states, double* actions, double* costs, double* total_return) {
  return CopyTrajectory(((mjpc_hip::CrossEntropyPlanner*)p)->BestTrajectory(), states, actions, nullptr, nullptr, costs, nullptr, total_return, nullptr);
}

// ---- SampleGradientPlanner
#define SGP(p) ((mjpc_hip::SampleGradientPlanner*)(p))
void* mjpc_sg_create(const MjpcHipModel* model, const MjpcHipTask* task, double exploration, int trajectories, int gradient_trajectories,
                     double gradient_filter, int representation, int spline_points, int max_samples, int max_horizon, int device) {
  auto* p = new mjpc_hip::SampleGradientPlanner();
  mjpc_hip::Numerics n;
  n.sampling_exploration[0] = exploration; n.sampling_trajectories = trajectories; n.sample_gradient_trajectories = gradient_trajectories;
  n.sample_gradient_filter = gradient_filter; n.sampling_representation = representation; n.sampling_spline_points = spline_points;
  n.max_samples = max_samples; n.max_horizon = max_horizon; n.device = device;
  p->Initialize(model, task, n);
  p->Allocate();
  return p;
}
void mjpc_sg_destroy(void* p) { delete SGP(p); }
void mjpc_sg_reset(void* p, int horizon, const double* a) { SGP(p)->Reset(horizon, a); }
void mjpc_sg_set_state(void* p, const double* s, const double* m, const double* u, double t) { SGP(p)->SetState(s, m, u, t); }
void mjpc_sg_set_task(void* p, const MjpcHipTask* task) { SGP(p)->SetTask(task); }
void mjpc_sg_set_seed(void* p, unsigned long long seed, unsigned long long it) { SGP(p)->seed = seed; SGP(p)->plan_iter = it; }
void mjpc_sg_set_noise(void* p, const double* eps) { SGP(p)->injected_noise_eps = eps; }
void mjpc_sg_set_counts(void* p, int trajectories, int gradient_trajectories) { SGP(p)->num_trajectory_ = trajectories; SGP(p)->num_gradient_ = gradient_trajectories; }
void mjpc_sg_optimize_policy(void* p, int horizon) { SGP(p)->OptimizePolicy(horizon); }
void mjpc_sg_nominal_trajectory(void* p, int horizon) { SGP(p)->NominalTrajectory(horizon); }
void mjpc_sg_action_from_policy(void* p, double* a, double t, int prev) { SGP(p)->ActionFromPolicy(a, nullptr, t, prev != 0); }
double mjpc_sg_improvement(void* p) { return SGP(p)->improvement; }
int mjpc_sg_winner(void* p) { return SGP(p)->winner; }
int mjpc_sg_winner_type(void* p) { return SGP(p)->winner_type_; }
int mjpc_sg_num_gradient(void* p) { return SGP(p)->num_gradient_; }
int mjpc_sg_num_parameters(void* p) { return SGP(p)->NumParameters(); }
void mjpc_sg_returns(void* p, double* out, int n) { std::copy(SGP(p)->returns.begin(), SGP(p)->returns.begin() + n, out); }
void mjpc_sg_trajectory_order(void* p, int* out, int n) { std::copy(SGP(p)->trajectory_order.begin(), SGP(p)->trajectory_order.begin() + n, out); }
void mjpc_sg_gradient(void* p, double* out, int n) { std::copy(SGP(p)->gradient.begin(), SGP(p)->gradient.begin() + n, out); }
int mjpc_sg_return_weight(void* p, double* out) { auto& w = SGP(p)->return_weight_; if (out) std::copy(w.begin(), w.end(), out); return (int)w.size(); }
int mjpc_sg_step_size(void* p, double* out) { auto& w = SGP(p)->step_size_; if (out) std::copy(w.begin(), w.end(), out); return (int)w.size(); }
int mjpc_sg_policy(void* p, double* times, double* values) { return mjpc_hip::CopyKnots(SGP(p)->policy, times, values); }
int mjpc_sg_candidate_policy(void* p, int index, double* times, double* values) { return SGP(p)->CandidatePolicy(index, times, values); }
int mjpc_sg_best_trajectory(void* p, double* states, double* actions, double* costs, double* total_return) {
  return CopyTrajectory(SGP(p)->BestTrajectory(), states, actions, nullptr, nullptr, costs, nullptr, total_return, nullptr);
}
void mjpc_sg_timings(void* p, double* noise, double* rollouts, double* update, double* gradient) {
  *noise = SGP(p)->noise_compute_time; *rollouts = SGP(p)->rollouts_compute_time; *update = SGP(p)->policy_update_compute_time;
  *gradient = SGP(p)->gradient_candidates_compute_time;
}
// host closed forms, no engine needed
void mjpc_sg_return_weights(const int* order, int num_noisy, double* weights) { mjpc_hip::SampleGradientPlanner::ReturnWeights(order, num_noisy, weights); }
void mjpc_sg_log_scale(double* values, double max_value, double min_value, int steps) { mjpc_hip::SampleGradientPlanner::LogScale(values, max_value, min_value, steps); }
#undef SGP

// ---- CostDerivatives, Gradient
void* mjpc_cd_create(int nd, int nu, int nr, int T) { auto* d = new mjpc_hip::CostDerivatives(); d->Allocate(nd, nu, nr, T); d->Reset(nd, nu, nr, T); return d; }
void mjpc_cd_destroy(void* cd) { delete (mjpc_hip::CostDerivatives*)cd; }
void mjpc_cd_reset(void* cd, int T) { auto* d = (mjpc_hip::CostDerivatives*)cd; d->Reset(d->dim_state_derivative, d->dim_action, d->dim_residual, T); }
int mjpc_cd_compute(void* cd, MjpcHipEngine* engine, const double* r, const double* rx, const double* ru, int T, int hessians) {
  auto* d = (mjpc_hip::CostDerivatives*)cd;
  return d->Compute(engine, r, rx, ru, d->dim_state_derivative, d->dim_action, d->dim_residual, T, hessians != 0) ? 0 : -1;
}
void mjpc_cd_blocks(void* cd, int T, double* cr, double* cx, double* cu, double* cxx, double* cuu, double* cxu) {
  auto* d = (mjpc_hip::CostDerivatives*)cd;
  const size_t nd = d->dim_state_derivative, nu = d->dim_action, nr = d->dim_residual, Tz = (size_t)T;
  if (T > d->horizon) return;
  if (cr) std::copy(d->cr.begin(), d->cr.begin() + Tz * nr, cr);
  if (cx) std::copy(d->cx.begin(), d->cx.begin() + Tz * nd, cx);
  if (cu) std::copy(d->cu.begin(), d->cu.begin() + Tz * nu, cu);
  if (cxx) std::copy(d->cxx.begin(), d->cxx.begin() + Tz * nd * nd, cxx);
  if (cuu) std::copy(d->cuu.begin(), d->cuu.begin() + Tz * nu * nu, cuu);
  if (cxu) std::copy(d->cxu.begin(), d->cxu.begin() + Tz * nd * nu, cxu);
}
int mjpc_gd_gradient_compute(int nd, int nu, int T, const double* A, const double* B, const double* cx, const double* cu, double* k, double* Vx,
                             double* Qx, double* Qu, double* dV) {
  mjpc_hip::Gradient g;
  if (T < 2) { g.Compute(nullptr, A, B, cx, cu, nd, nu, T); return -1; }
  std::vector<double> kk((size_t)T * nu + 1);
  const int rc = g.Compute(kk.data(), A, B, cx, cu, nd, nu, T);
  const size_t Tz = (size_t)T;
  if (k) std::copy(kk.begin(), kk.begin() + Tz * nu, k);
  if (Vx) std::copy(g.Vx.begin(), g.Vx.begin() + Tz * nd, Vx);
  if (Qx) std::copy(g.Qx.begin(), g.Qx.begin() + (Tz - 1) * nd, Qx);
  if (Qu) std::copy(g.Qu.begin(), g.Qu.begin() + (Tz - 1) * nu, Qu);
  if (dV) { dV[0] = g.dV[0]; dV[1] = g.dV[1]; }
  return rc;
}

// ---- GradientPlanner
#define GDP(p) ((mjpc_hip::GradientPlanner*)(p))
void* mjpc_gd_create(const MjpcHipModel* model, const MjpcHipTask* task, int num_trajectory, int spline_points, int representation, int derivative_skip,
                     int max_rollout, double min_linesearch_step, double fd_tolerance, int fd_mode, int max_samples, int max_horizon, int device) {
  auto* p = new mjpc_hip::GradientPlanner();
  mjpc_hip::Numerics n;
  n.gradient_num_trajectory = num_trajectory; n.gradient_spline_points = spline_points; n.gradient_representation = representation;
  n.derivative_skip = derivative_skip; n.max_samples = max_samples; n.max_horizon = max_horizon; n.device = device;
  p->settings.max_rollout = max_rollout; p->settings.min_linesearch_step = min_linesearch_step; p->settings.fd_tolerance = fd_tolerance; p->settings.fd_mode = fd_mode;
  p->Initialize(model, task, n);
  p->Allocate();
  return p;
}
void mjpc_gd_destroy(void* p) { delete GDP(p); }
void mjpc_gd_reset(void* p, int horizon, const double* a) { GDP(p)->Reset(horizon, a); }
void mjpc_gd_set_state(void* p, const double* s, const double* m, const double* u, double t) { GDP(p)->SetState(s, m, u, t); }
void mjpc_gd_set_task(void* p, const MjpcHipTask* task) { GDP(p)->SetTask(task); }
void mjpc_gd_set_num_trajectory(void* p, int n) { GDP(p)->num_trajectory = n; }
void mjpc_gd_optimize_policy(void* p, int horizon) { GDP(p)->OptimizePolicy(horizon); }
void mjpc_gd_nominal_trajectory(void* p, int horizon) { GDP(p)->NominalTrajectory(horizon); }
void mjpc_gd_action_from_policy(void* p, double* a, double t, int prev) { GDP(p)->ActionFromPolicy(a, nullptr, t, prev != 0); }
double mjpc_gd_improvement(void* p) { return GDP(p)->improvement; }
int mjpc_gd_policy(void* p, double* times, double* values) {
  const mjpc_hip::GradientPolicy& pol = GDP(p)->policy;
  if (times) std::copy(pol.times.begin(), pol.times.begin() + pol.num_spline_points, times);
  if (values) std::copy(pol.parameters.begin(), pol.parameters.begin() + (size_t)pol.num_spline_points * pol.nu, values);
  return pol.num_spline_points;
}
void mjpc_gd_set_policy(void* p, const double* times, const double* values) {
  mjpc_hip::GradientPolicy& pol = GDP(p)->policy;
  std::copy(times, times + pol.num_spline_points, pol.times.begin());
  std::copy(values, values + (size_t)pol.num_spline_points * pol.nu, pol.parameters.begin());
}
int mjpc_gd_best_trajectory(void* p, double* states, double* actions, double* costs, double* total_return) {
  return CopyTrajectory(GDP(p)->BestTrajectory(), states, actions, nullptr, nullptr, costs, nullptr, total_return, nullptr);
}
void mjpc_gd_values(void* p, double* out) {
  auto* g = GDP(p);
  out[0] = g->action_step; out[1] = g->expected; out[2] = g->improvement; out[3] = g->surprise; out[4] = g->winner; out[5] = g->failed ? 1 : 0;
}
void mjpc_gd_timings(void* p, double* out) {
  auto* g = GDP(p);
  out[0] = g->nominal_compute_time; out[1] = g->derivative_compute_time; out[2] = g->gradient_compute_time; out[3] = g->rollouts_compute_time;
  out[4] = g->policy_update_compute_time;
}
void mjpc_gd_returns(void* p, double* out, int n) { std::copy(GDP(p)->returns.begin(), GDP(p)->returns.begin() + std::min(n, (int)GDP(p)->returns.size()), out); }
int mjpc_gd_linesearch_steps(void* p, double* out) { auto& w = GDP(p)->linesearch_steps; if (out) std::copy(w.begin(), w.end(), out); return (int)w.size(); }
int mjpc_gd_parameter_update(void* p, double* out) {
  auto& pol = GDP(p)->nominal_policy; const int n = pol.num_spline_points * pol.nu;
  if (out) std::copy(pol.parameter_update.begin(), pol.parameter_update.begin() + n, out);
  return n;
}
void mjpc_gd_spline_mapping(int representation, int dim, const double* input_times, int num_input, const double* output_times, int num_output, double* mapping) {
  if (num_input > mjpc_hip::kMaxGradientSplinePoints || num_output > mjpc_hip::kMaxTrajectoryHorizon || representation < 0 || representation > 2) {
    mjpc_hip::GradientPlanner::Refuse("mjpc_gd_spline_mapping: representation 0..2, at most 25 inputs and kMaxTrajectoryHorizon outputs"); return; }
  std::unique_ptr<mjpc_hip::SplineMapping> m;
  if (representation == 0) m.reset(new mjpc_hip::ZeroSplineMapping()); else if (representation == 1) m.reset(new mjpc_hip::LinearSplineMapping());
  else m.reset(new mjpc_hip::CubicSplineMapping());
  m->Allocate(dim);
  m->Compute(std::vector<double>(input_times, input_times + num_input), num_input, output_times, num_output);
  std::copy(m->mapping.begin(), m->mapping.begin() + (size_t)(dim * num_output) * (dim * num_input), mapping);
}
void mjpc_gd_policy_action(int representation, int nu, const double* ctrlrange, const double* times, const double* parameters, int num_spline_points, double time,
                           double* action) {
  mjpc_hip::GradientPolicy pol;
  pol.nu = nu; pol.ctrlrange.assign(ctrlrange, ctrlrange + 2 * nu); pol.representation = representation; pol.num_spline_points = num_spline_points;
  pol.times.assign(times, times + num_spline_points); pol.parameters.assign(parameters, parameters + (size_t)num_spline_points * nu);
  pol.Action(action, nullptr, time);
}

// ---- iLQGPlanner
#define ILQ(p) ((mjpc_hip::iLQGPlanner*)(p))
void* mjpc_ilqg_create(const MjpcHipModel* model, const MjpcHipTask* task, int num_trajectory, int representation, int derivative_skip, int fused,
                       const double* settings, int max_samples, int max_horizon, int device) {
  auto* p = new mjpc_hip::iLQGPlanner();
  mjpc_hip::Numerics n;
  n.derivative_skip = derivative_skip; n.max_samples = max_samples; n.max_horizon = max_horizon; n.device = device;
  p->num_trajectory = num_trajectory; p->representation = representation; p->fused = fused != 0;
  if (settings) {
    mjpc_hip::iLQGSettings& s = p->settings;
    s.min_linesearch_step = settings[0]; s.fd_tolerance = settings[1]; s.fd_mode = settings[2]; s.min_regularization = settings[3];
    s.max_regularization = settings[4]; s.regularization_type = (int)settings[5]; s.max_regularization_iterations = (int)settings[6];
    s.action_limits = (int)settings[7]; s.nominal_feedback_scaling = (int)settings[8];
  }
  p->Initialize(model, task, n);
  p->Allocate();
  return p;
}
void mjpc_ilqg_destroy(void* p) { delete ILQ(p); }
void mjpc_ilqg_reset(void* p, int horizon, const double* a) { ILQ(p)->Reset(horizon, a); }
void mjpc_ilqg_set_state(void* p, const double* s, const double* m, const double* u, double t) { ILQ(p)->SetState(s, m, u, t); }
void mjpc_ilqg_set_task(void* p, const MjpcHipTask* task) { ILQ(p)->SetTask(task); }
void mjpc_ilqg_set_num_trajectory(void* p, int n) { ILQ(p)->num_trajectory = n; }
void mjpc_ilqg_optimize_policy(void* p, int horizon) { ILQ(p)->OptimizePolicy(horizon); }
void mjpc_ilqg_nominal_trajectory(void* p, int horizon) { ILQ(p)->NominalTrajectory(horizon); }
void mjpc_ilqg_iteration(void* p, int horizon) { ILQ(p)->Iteration(horizon); }
void mjpc_ilqg_action_from_policy(void* p, double* a, const double* state, double t, int prev) { ILQ(p)->ActionFromPolicy(a, state, t, prev != 0); }
double mjpc_ilqg_improvement(void* p) { return ILQ(p)->improvement; }
int mjpc_ilqg_best_trajectory(void* p, double* states, double* actions, double* costs, double* total_return) {
  return CopyTrajectory(ILQ(p)->BestTrajectory(), states, actions, nullptr, nullptr, costs, nullptr, total_return, nullptr);
}
void mjpc_ilqg_values(void* p, double* out) {
  auto* g = ILQ(p);
  out[0] = g->action_step; out[1] = g->expected; out[2] = g->improvement; out[3] = g->surprise; out[4] = g->winner; out[5] = g->backward_pass_failed ? 1 : 0;
  out[6] = g->feedback_scaling; out[7] = g->backward_pass.regularization; out[8] = g->backward_pass.regularization_rate; out[9] = g->all_failed ? 1 : 0;
  out[10] = g->backward_pass.dV[0]; out[11] = g->backward_pass.dV[1];
}
void mjpc_ilqg_timings(void* p, double* out) {
  auto* g = ILQ(p);
  out[0] = g->nominal_compute_time; out[1] = g->derivative_compute_time; out[2] = g->rollouts_compute_time; out[3] = g->policy_update_compute_time;
  out[4] = g->resample_kernel_time; out[5] = g->rollout_kernel_time;
}
void mjpc_ilqg_returns(void* p, double* out, int n) { std::copy(ILQ(p)->returns.begin(), ILQ(p)->returns.begin() + std::min(n, (int)ILQ(p)->returns.size()), out); }
int mjpc_ilqg_linesearch_steps(void* p, double* out) { auto& w = ILQ(p)->linesearch_steps; if (out) std::copy(w.begin(), w.end(), out); return (int)w.size(); }
// which: 0 policy, 1 previous_policy, 2 candidate.  Arrays of `horizon` knots (any may be NULL); returns the policy's trajectory.horizon
int mjpc_ilqg_get_policy(void* p, int which, double* times, double* states, double* actions, double* feedback_gain, double* action_improvement,
                         double* feedback_scaling) {
  auto* g = ILQ(p);
  const mjpc_hip::iLQGPolicy& pol = which == 0 ? g->policy : which == 1 ? g->previous_policy : g->candidate;
  const size_t H = pol.trajectory.horizon, ds = pol.nq + pol.nv + pol.na, nd = 2 * pol.nv + pol.na, nu = pol.nu;
  if (times) std::copy(pol.trajectory.times.begin(), pol.trajectory.times.begin() + H, times);
  if (states) std::copy(pol.trajectory.states.begin(), pol.trajectory.states.begin() + H * ds, states);
  if (actions) std::copy(pol.trajectory.actions.begin(), pol.trajectory.actions.begin() + H * nu, actions);
  if (feedback_gain) std::copy(pol.feedback_gain.begin(), pol.feedback_gain.begin() + H * nu * nd, feedback_gain);
  if (action_improvement) std::copy(pol.action_improvement.begin(), pol.action_improvement.begin() + H * nu, action_improvement);
  if (feedback_scaling) *feedback_scaling = pol.feedback_scaling;
  return (int)H;
}
int mjpc_ilqg_best_rollout(const double* returns, const int* failures, int n) { return mjpc_hip::iLQGPlanner::BestRollout(returns, failures, n); }

// ---- iLQSPlanner
#define ILS(p) ((mjpc_hip::iLQSPlanner*)(p))
void* mjpc_ilqs_create(const MjpcHipModel* model, const MjpcHipTask* task, const double* exploration, int trajectories, int representation, int sliding_plan,
                       int spline_points, int ilqg_num_trajectory, int ilqg_representation, int derivative_skip, int fused, const double* settings,
                       int max_samples, int max_horizon, int device) {
  auto* p = new mjpc_hip::iLQSPlanner();
  mjpc_hip::Numerics n;
  n.sampling_exploration[0] = exploration[0]; n.sampling_exploration[1] = exploration[1];
  n.sampling_trajectories = trajectories; n.sampling_representation = representation; n.sampling_sliding_plan = sliding_plan;
  n.sampling_spline_points = spline_points; n.derivative_skip = derivative_skip; n.max_samples = max_samples; n.max_horizon = max_horizon; n.device = device;
  p->ilqg.num_trajectory = ilqg_num_trajectory; p->ilqg.representation = ilqg_representation; p->ilqg.fused = fused != 0;
  if (settings) {
    mjpc_hip::iLQGSettings& s = p->ilqg.settings;
    s.min_linesearch_step = settings[0]; s.fd_tolerance = settings[1]; s.fd_mode = settings[2]; s.min_regularization = settings[3];
    s.max_regularization = settings[4]; s.regularization_type = (int)settings[5]; s.max_regularization_iterations = (int)settings[6];
    s.action_limits = (int)settings[7]; s.nominal_feedback_scaling = (int)settings[8];
  }
  p->Initialize(model, task, n);
  p->Allocate();
  return p;
}
void mjpc_ilqs_destroy(void* p) { delete ILS(p); }
void mjpc_ilqs_reset(void* p, int horizon, const double* a) { ILS(p)->Reset(horizon, a); }
void mjpc_ilqs_set_state(void* p, const double* s, const double* m, const double* u, double t) { ILS(p)->SetState(s, m, u, t); }
void mjpc_ilqs_set_task(void* p, const MjpcHipTask* task) { ILS(p)->SetTask(task); }
void mjpc_ilqs_optimize_policy(void* p, int horizon) { ILS(p)->OptimizePolicy(horizon); }
void mjpc_ilqs_nominal_trajectory(void* p, int horizon) { ILS(p)->NominalTrajectory(horizon); }
void mjpc_ilqs_action_from_policy(void* p, double* a, const double* state, double t, int prev) { ILS(p)->ActionFromPolicy(a, state, t, prev != 0); }
int mjpc_ilqs_best_trajectory(void* p, double* states, double* actions, double* costs, double* total_return) {
  return CopyTrajectory(ILS(p)->BestTrajectory(), states, actions, nullptr, nullptr, costs, nullptr, total_return, nullptr);
}
void mjpc_ilqs_values(void* p, int* out) {
  auto* g = ILS(p);
  out[0] = g->active_policy; out[1] = g->previous_active_policy; out[2] = g->converted ? 1 : 0; out[3] = g->returned_early ? 1 : 0;
  out[4] = g->iterated ? 1 : 0; out[5] = (g->iterated && g->ilqg.adopted) ? 1 : 0;
}
void mjpc_ilqs_timings(void* p, double* out) { out[0] = ILS(p)->fit_compute_time; out[1] = ILS(p)->fit_cache_miss ? 1.0 : 0.0; }
void mjpc_ilqs_set_noise_exploration(void* p, double first, double second) { ILS(p)->sampling.noise_exploration[0] = first; ILS(p)->sampling.noise_exploration[1] = second; }
void* mjpc_ilqs_sampling(void* p) { return &ILS(p)->sampling; }
void* mjpc_ilqs_ilqg(void* p) { return &ILS(p)->ilqg; }
int mjpc_ilqs_fitted_knots(void* p, double* times, double* values) {
  auto* g = ILS(p);
  if (times) std::copy(g->spline_times_cache.begin(), g->spline_times_cache.end(), times);
  if (values) std::copy(g->spline_parameters_cache.begin(), g->spline_parameters_cache.end(), values);
  return (int)g->spline_times_cache.size();
}
int mjpc_ilqs_sampling_member(void* p, int index, double* states, double* actions, double* times, double* residual, double* total_return) {
  mjpc_hip::SamplingPlanner& s = ILS(p)->sampling;
  if (index < 0 || index >= s.num_trajectory_ || s.winner < 0) return 0;
  s.FetchCandidateUnranked(index);
  const int H = CopyTrajectory(&s.trajectory_winner, states, actions, times, residual, nullptr, nullptr, total_return, nullptr);
  if (s.winner != index) s.FetchCandidateUnranked(s.winner);
  return H;
}
int mjpc_ilqs_action_source(int previous_active_policy, int active_policy, int use_previous) {
  return mjpc_hip::iLQSPlanner::ActionSource(previous_active_policy, active_policy, use_previous != 0);
}
int mjpc_ilqs_spline_fit(int representation, int P, const double* knot_times, int H1, const double* action_times, int nu, const double* actions,
                         double* out_knots) {
  return mjpc_hip::SplineFit(representation, P, knot_times, H1, action_times, nu, actions, out_knots);
}
#undef ILS

// ---- Kalman, Unscented
namespace {
void EstimatorSettingsFrom(mjpc_hip::EstimatorSettings& s, const double* v) {
  if (!v) return;
  s.epsilon = v[0]; s.flg_centered = v[1] != 0; s.alpha = v[2]; s.beta = v[3];
  s.covariance_initial_scale = v[4]; s.process_noise_scale = v[5]; s.sensor_noise_scale = v[6];
}
}  // namespace
#define EST(p) ((mjpc_hip::Estimator*)(p))
void* mjpc_kalman_create(MjpcHipEngine* engine, const MjpcHipModel* model, const MjpcHipTask* task, int sensor_first_row, int num_sensor,
                         const double* settings) {
  auto* k = new mjpc_hip::Kalman();
  mjpc_hip::EstimatorSettings s; EstimatorSettingsFrom(s, settings);
  if (k->Initialize(engine, model, task, sensor_first_row, num_sensor, s) != 0) { delete k; return nullptr; }
  return (mjpc_hip::Estimator*)k;
}
void mjpc_kalman_destroy(void* p) { delete (mjpc_hip::Kalman*)EST(p); }
int mjpc_kalman_update_measurement(void* p, const double* ctrl, const double* sensor) { return ((mjpc_hip::Kalman*)EST(p))->UpdateMeasurement(ctrl, sensor); }
int mjpc_kalman_update_prediction(void* p) { return ((mjpc_hip::Kalman*)EST(p))->UpdatePrediction(); }
int mjpc_kalman_update(void* p, const double* ctrl, const double* sensor) { return ((mjpc_hip::Kalman*)EST(p))->Update(ctrl, sensor); }
void* mjpc_unscented_create(MjpcHipEngine* engine, const MjpcHipModel* model, const MjpcHipTask* task, int sensor_first_row, int num_sensor,
                            const double* settings) {
  auto* u = new mjpc_hip::Unscented();
  mjpc_hip::EstimatorSettings s; EstimatorSettingsFrom(s, settings);
  if (u->Initialize(engine, model, task, sensor_first_row, num_sensor, s) != 0) { delete u; return nullptr; }
  return (mjpc_hip::Estimator*)u;
}
void mjpc_unscented_destroy(void* p) { delete (mjpc_hip::Unscented*)EST(p); }
int mjpc_unscented_update(void* p, const double* ctrl, const double* sensor) { return ((mjpc_hip::Unscented*)EST(p))->Update(ctrl, sensor); }
void mjpc_unscented_weights(void* p, double* out) {
  auto* u = (mjpc_hip::Unscented*)EST(p);
  out[0] = u->sigma_step; out[1] = u->weight_mean0; out[2] = u->weight_covariance0; out[3] = u->weight_sigma;
}
void mjpc_estimator_reset(void* p, const double* state, double time) { EST(p)->Reset(state, time); }
void mjpc_estimator_set_shared(void* p, const double* mocap, const double* userdata) { EST(p)->SetShared(mocap, userdata); }
void mjpc_estimator_dims(void* p, int* out) { auto* e = EST(p); out[0] = e->nq + e->nv + e->na; out[1] = e->nd; out[2] = e->ns; out[3] = e->last_failure; }
double mjpc_estimator_time(void* p, const double* set) { if (set) EST(p)->time = *set; return EST(p)->time; }
void mjpc_estimator_access(void* p, int which, const double* set, double* out) {
  auto* e = EST(p);
  std::vector<double>* v[4] = {&e->state, &e->covariance, &e->noise_process, &e->noise_sensor};
  if (which < 0 || which > 3) return;
  if (set) std::copy(set, set + v[which]->size(), v[which]->begin());
  if (out) std::copy(v[which]->begin(), v[which]->end(), out);
}
#undef EST
int mjpc_estimator_covariance_factor(int n, const double* P, double* L) { return mjpc_hip::CovarianceFactor(n, P, L) ? 0 : mjpc_hip::kEstimatorCovarianceRank; }
int mjpc_estimator_kalman_gain(int nd, int ns, const double* P, const double* C, const double* R, double* PCt, double* factor, double* gain) {
  return mjpc_hip::KalmanGain(nd, ns, P, C, R, PCt, factor, gain);
}
void mjpc_estimator_kalman_correct(int nd, int ns, const double* PCt, const double* factor, const double* gain, const double* sensor_error,
                                   double* correction, double* P) {
  mjpc_hip::KalmanCorrect(nd, ns, PCt, factor, gain, sensor_error, correction, P);
}
void mjpc_estimator_covariance_predict(int nd, const double* A, const double* Q, double* P) { mjpc_hip::CovariancePredict(nd, A, Q, P); }
int mjpc_estimator_unscented_correct(int nd, int ns, const double* cov_ss, const double* cov_sy, const double* cov_yy, const double* sensor_error,
                                     double* correction, double* P) {
  return mjpc_hip::UnscentedCorrect(nd, ns, cov_ss, cov_sy, cov_yy, sensor_error, correction, P);
}

// ---- iLQGBackwardPass, BoxQP, iLQGPolicy
namespace {
struct IlqgBp {
  mjpc_hip::iLQGBackwardPass bp;
  mjpc_hip::BoxQP qp;
  mjpc_hip::iLQGPolicy policy;
  mjpc_hip::ModelDerivatives md;
  mjpc_hip::CostDerivatives cd;
  int n = 0, m = 0;
  void Rows(int T) {
    policy.nu = m;
    policy.action_improvement.assign((size_t)m * T, 0.0); policy.feedback_gain.assign((size_t)m * n * T, 0.0);
  }
  void Load(int T, const double* A, const double* B, const double* cx, const double* cu, const double* cxx, const double* cxu, const double* cuu) {
    const size_t Tz = T, nn = (size_t)n * n, nm = (size_t)n * m, mm = (size_t)m * m;
    md.A.assign(A, A + (Tz - 1) * nn); md.B.assign(B, B + (Tz - 1) * nm);
    cd.cx.assign(cx, cx + Tz * n); cd.cu.assign(cu, cu + Tz * m); cd.cxx.assign(cxx, cxx + Tz * nn); cd.cxu.assign(cxu, cxu + Tz * nm); cd.cuu.assign(cuu, cuu + Tz * mm);
  }
  void Out(int T, double* k, double* K) {
    if (k) std::copy(policy.action_improvement.begin(), policy.action_improvement.begin() + (size_t)m * T, k);
    if (K) std::copy(policy.feedback_gain.begin(), policy.feedback_gain.begin() + (size_t)m * n * T, K);
  }
  static mjpc_hip::iLQGSettings Settings(const int* si, const double* sd) {
    mjpc_hip::iLQGSettings s;
    s.regularization_type = si[0]; s.action_limits = si[1]; s.max_regularization_iterations = si[2];
    s.min_regularization = sd[0]; s.max_regularization = sd[1];
    return s;
  }
  // Reset keeps the object's regularisation: the C view's reset is the only place that restores the defaults
  void Zero(int T) {
    const double r = bp.regularization, rr = bp.regularization_rate, f = bp.regularization_factor;
    bp.Reset(n, m, T);
    bp.regularization = r; bp.regularization_rate = rr; bp.regularization_factor = f;
  }
};
}  // namespace
#define IBP(p) ((IlqgBp*)(p))
void* mjpc_ilqg_bp_create(int nd, int nu, int T) {
  auto* d = new IlqgBp();
  d->n = nd; d->m = nu;
  d->bp.Allocate(nd, nu, T); d->bp.Reset(nd, nu, T); d->qp.Allocate(nu);
  return d;
}
void mjpc_ilqg_bp_destroy(void* p) { delete IBP(p); }
void mjpc_ilqg_bp_reset(void* p, int T) { IBP(p)->bp.Reset(IBP(p)->n, IBP(p)->m, T); IBP(p)->qp.Allocate(IBP(p)->m); }
void mjpc_ilqg_bp_riccati_host(void* p, int T, const double* A, const double* B, const double* cx, const double* cu, const double* cxx, const double* cxu,
                               const double* cuu, const double* actions, const double* action_limits, const int* si, const double* sd, double* k, double* K,
                               int* status) {
  IlqgBp* d = IBP(p);
  if (T < 2) { d->bp.RiccatiRegularized(nullptr, nullptr, A, B, cx, cu, cxx, cxu, cuu, d->n, d->m, T, d->qp, actions, action_limits, IlqgBp::Settings(si, sd), status); return; }
  d->Zero(T); d->Rows(T);
  d->bp.RiccatiRegularized(d->policy.action_improvement.data(), d->policy.feedback_gain.data(), A, B, cx, cu, cxx, cxu, cuu, d->n, d->m, T, d->qp, actions,
                           action_limits, IlqgBp::Settings(si, sd), status);
  d->Out(T, k, K);
}
int mjpc_ilqg_bp_riccati(void* p, int T, double reg, const double* A, const double* B, const double* cx, const double* cu, const double* cxx, const double* cxu,
                         const double* cuu, const double* actions, const double* action_limits, const int* si, const double* sd, double* k, double* K) {
  IlqgBp* d = IBP(p);
  if (T < 2) return d->bp.Riccati(nullptr, nullptr, nullptr, d->n, d->m, T, reg, d->qp, actions, action_limits, IlqgBp::Settings(si, sd));
  d->Zero(T); d->Rows(T); d->Load(T, A, B, cx, cu, cxx, cxu, cuu);
  const int rc = d->bp.Riccati(&d->policy, &d->md, &d->cd, d->n, d->m, T, reg, d->qp, actions, action_limits, IlqgBp::Settings(si, sd));
  d->Out(T, k, K);
  return rc;
}
int mjpc_ilqg_bp_compute(void* p, MjpcHipEngine* engine, int T, const double* A, const double* B, const double* cx, const double* cu, const double* cxx,
                         const double* cxu, const double* cuu, const double* actions, const double* action_limits, const int* si, const double* sd, double* k,
                         double* K, int* status) {
  IlqgBp* d = IBP(p);
  if (T < 2 || !A || !B || !cx || !cu || !cxx || !cxu || !cuu) {        // the engine names the error
    MjpcHipRiccatiSettings s;
    s.struct_size = (int)sizeof(s); s.regularization_type = si[0]; s.action_limits = si[1]; s.max_regularization_iterations = si[2];
    s.min_regularization = sd[0]; s.max_regularization = sd[1]; s.regularization_factor = d->bp.regularization_factor;
    return mjpc_hip_ilqg_backward_pass(engine, T, d->n, d->m, A, B, cx, cu, cxx, cxu, cuu, actions, action_limits, &s, &d->bp.regularization,
                                       &d->bp.regularization_rate, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, status);
  }
  d->Rows(T); d->Load(T, A, B, cx, cu, cxx, cxu, cuu);
  const bool ok = d->bp.Compute(engine, &d->policy, &d->md, &d->cd, d->n, d->m, T, actions, action_limits, IlqgBp::Settings(si, sd), status);
  d->Out(T, k, K);
  return ok ? 0 : -1;
}
int mjpc_ilqg_bp_compute_fused(void* p, MjpcHipEngine* engine, int T, const double* x, const double* u, const double* h, const double* residual,
                               const double* mocap, const double* userdata, double fd_tolerance, int fd_mode, const int* si, const double* sd, double* k,
                               double* K, int* status, int* failure) {
  IlqgBp* d = IBP(p);
  mjpc_hip::iLQGSettings s = IlqgBp::Settings(si, sd);
  s.fd_tolerance = fd_tolerance; s.fd_mode = fd_mode;
  d->Rows(T > 0 ? T : 1);
  const bool ok = d->bp.ComputeFused(engine, &d->policy, x, u, h, residual, d->n, d->m, T > 0 ? T : 1, s, status, failure, mocap, userdata);
  if (ok) d->Out(T, k, K);
  return ok ? 0 : -1;
}
void mjpc_ilqg_bp_blocks(void* p, int T, double* Vx, double* Vxx, double* Qx, double* Qu, double* Qxx, double* Qxu, double* Quu, double* dV) {
  IlqgBp* d = IBP(p);
  const size_t Tz = T, n = d->n, m = d->m;
  if (d->bp.Vx.size() < Tz * n || T < 1) return;
  if (Vx) std::copy(d->bp.Vx.begin(), d->bp.Vx.begin() + Tz * n, Vx);
  if (Vxx) std::copy(d->bp.Vxx.begin(), d->bp.Vxx.begin() + Tz * n * n, Vxx);
  if (Qx) std::copy(d->bp.Qx.begin(), d->bp.Qx.begin() + (Tz - 1) * n, Qx);
  if (Qu) std::copy(d->bp.Qu.begin(), d->bp.Qu.begin() + (Tz - 1) * m, Qu);
  if (Qxx) std::copy(d->bp.Qxx.begin(), d->bp.Qxx.begin() + (Tz - 1) * n * n, Qxx);
  if (Qxu) std::copy(d->bp.Qxu.begin(), d->bp.Qxu.begin() + (Tz - 1) * n * m, Qxu);
  if (Quu) std::copy(d->bp.Quu.begin(), d->bp.Quu.begin() + (Tz - 1) * m * m, Quu);
  if (dV) { dV[0] = d->bp.dV[0]; dV[1] = d->bp.dV[1]; }
}
void mjpc_ilqg_bp_regularization(void* p, const double* set, double* out) {
  auto& b = IBP(p)->bp;
  if (set) { b.regularization = set[0]; b.regularization_rate = set[1]; b.regularization_factor = set[2]; }
  if (out) { out[0] = b.regularization; out[1] = b.regularization_rate; out[2] = b.regularization_factor; }
}
void mjpc_ilqg_bp_scale_regularization(void* p, double factor, double reg_min, double reg_max) { IBP(p)->bp.ScaleRegularization(factor, reg_min, reg_max); }
void mjpc_ilqg_bp_update_regularization(void* p, double reg_min, double reg_max, double z, double s) { IBP(p)->bp.UpdateRegularization(reg_min, reg_max, z, s); }
#undef IBP
int mjpc_ilqg_boxqp(int n, const double* H, const double* g, const double* lower, const double* upper, double* res, double* R, int* index) {
  return mjpc_hip::BoxQPSolve(res, R, index, H, g, n, lower, upper);
}
void mjpc_ilqg_policy_action(int nq, int nv, int na, int nu, int njnt, const int* jnt_type, const int* jnt_qposadr, const int* jnt_dofadr, const double* ctrlrange,
                             int representation, int horizon, const double* times, const double* states, const double* actions, const double* feedback_gain,
                             double feedback_scaling, const double* state, double time, double* action) {
  mjpc_hip::iLQGPolicy p;
  p.Allocate(nq, nv, na, nu, njnt, jnt_type, jnt_qposadr, jnt_dofadr, ctrlrange, 0, 0, horizon, representation);
  const size_t H = horizon, ds = nq + nv + na, nd = 2 * nv + na;
  p.trajectory.times.assign(times, times + H);
  p.trajectory.states.assign(states, states + H * ds);
  p.trajectory.actions.assign(actions, actions + H * nu);
  p.feedback_gain.assign(feedback_gain, feedback_gain + H * nu * nd);
  p.feedback_scaling = feedback_scaling;
  p.Action(action, state, time);
}

// ---- InverseDerivatives
void* mjpc_id_create(int dim_state, int nq, int nv, int nu, int nr, int T) { auto* d = new mjpc_hip::InverseDerivatives(); d->Allocate(dim_state, nq, nv, nu, nr, T); d->Reset(T); return d; }
void mjpc_id_destroy(void* id) { delete (mjpc_hip::InverseDerivatives*)id; }
void mjpc_id_set_row_stages(void* id, const int* stage) { ((mjpc_hip::InverseDerivatives*)id)->SetRowStages(stage); }
int mjpc_id_row_stages_from_table(void* id, const MjpcHipTask* task) {
  auto* d = (mjpc_hip::InverseDerivatives*)id;
  if (!task || task->num_residual != d->dim_sensor) return -1;
  std::vector<int> st(d->dim_sensor + 1);
  if (!mjpc_hip::InverseDerivatives::RowStagesFromTable(task, st.data())) return -1;
  d->SetRowStages(st.data());
  return 0;
}
void mjpc_id_row_stages(void* id, int* stage) { auto* d = (mjpc_hip::InverseDerivatives*)id; std::copy(d->row_stage.begin(), d->row_stage.end(), stage); }
int mjpc_id_compute(void* id, MjpcHipEngine* engine, const double* x, const double* u, const double* a, const double* h, int T, double tol, int mode,
                    int discrete, const double* mocap, const double* userdata) {
  return ((mjpc_hip::InverseDerivatives*)id)->Compute(engine, x, u, a, h, T, tol, mode, discrete, mocap, userdata) ? 0 : -1;
}
void mjpc_id_blocks(void* id, int T, double* DfDq, double* DfDv, double* DfDa, double* DsDq, double* DsDv, double* DsDa, int* failure) {
  auto* d = (mjpc_hip::InverseDerivatives*)id;
  const size_t nf = (size_t)T * d->dim_v * d->dim_v, ns = (size_t)T * d->dim_sensor * d->dim_v;
  double* out[6] = {DfDq, DfDv, DfDa, DsDq, DsDv, DsDa};
  const std::vector<double>* src[6] = {&d->DfDq, &d->DfDv, &d->DfDa, &d->DsDq, &d->DsDv, &d->DsDa};
  for (int k = 0; k < 6; k++) if (out[k]) std::copy(src[k]->begin(), src[k]->begin() + (k < 3 ? nf : ns), out[k]);
  if (failure) std::copy(d->failure.begin(), d->failure.begin() + T, failure);
}

// ---- ModelDerivatives
void* mjpc_md_create(int dim_state, int nd, int nu, int nr, int T) { auto* d = new mjpc_hip::ModelDerivatives(); d->Allocate(nd, nu, nr, T, dim_state); d->Reset(nd, nu, nr, T); return d; }
void mjpc_md_destroy(void* md) { delete (mjpc_hip::ModelDerivatives*)md; }
void mjpc_md_reset(void* md, int T) { auto* d = (mjpc_hip::ModelDerivatives*)md; d->Reset(d->dim_state_derivative, d->dim_action, d->dim_sensor, T); }
int mjpc_md_compute(void* md, MjpcHipEngine* engine, const double* x, const double* u, const double* h, int T, double tol, int mode, int skip,
                    const double* mocap, const double* userdata) {
  return ((mjpc_hip::ModelDerivatives*)md)->Compute(engine, x, u, h, T, tol, mode, skip, mocap, userdata) ? 0 : -1;
}
void mjpc_md_index_sets(void* md, int T, int skip) { ((mjpc_hip::ModelDerivatives*)md)->IndexSets(T, skip); }
void mjpc_md_interpolate(void* md) { ((mjpc_hip::ModelDerivatives*)md)->Interpolate(); }
void mjpc_md_indices(void* md, int* evaluate, int* interpolate, int* n) {
  auto* d = (mjpc_hip::ModelDerivatives*)md;
  if (evaluate) std::copy(d->evaluate_.begin(), d->evaluate_.end(), evaluate);
  if (interpolate) std::copy(d->interpolate_.begin(), d->interpolate_.end(), interpolate);
  if (n) { n[0] = (int)d->evaluate_.size(); n[1] = (int)d->interpolate_.size(); }
}
void mjpc_md_blocks(void* md, int T, int store, double* A, double* B, double* C, double* D, int* failure) {
  auto* d = (mjpc_hip::ModelDerivatives*)md;
  const size_t nd = d->dim_state_derivative, nu = d->dim_action, nr = d->dim_sensor, n = (size_t)T;
  if (n > d->failure.size()) return;
  double* user[4] = {A, B, C, D};
  std::vector<double>* own[4] = {&d->A, &d->B, &d->C, &d->D};
  const size_t cnt[4] = {n * nd * nd, n * nd * nu, n * nr * nd, n * nr * nu};
  for (int k = 0; k < 4; k++) {
    if (!user[k]) continue;
    if (store) std::copy(user[k], user[k] + cnt[k], own[k]->begin()); else std::copy(own[k]->begin(), own[k]->begin() + cnt[k], user[k]);
  }
  if (failure) { if (store) std::copy(failure, failure + n, d->failure.begin()); else std::copy(d->failure.begin(), d->failure.begin() + n, failure); }
}

// ---- RobustPlanner
void* mjpc_robust_create(const MjpcHipModel* model, const MjpcHipTask* task, const double* exploration, int trajectories, int representation,
                         int spline_points, int repetitions, int candidates, double xfrc_std, double xfrc_rate, int max_samples, int max_horizon,
                         int device) {
  auto* p = new mjpc_hip::RobustPlanner();
  mjpc_hip::Numerics n;
  n.sampling_exploration[0] = exploration[0]; n.sampling_exploration[1] = exploration[1];
  n.sampling_trajectories = trajectories; n.sampling_representation = representation; n.sampling_spline_points = spline_points;
  n.robust_repetitions = repetitions; n.robust_candidates = candidates; n.robust_xfrc = xfrc_std; n.robust_xfrc_rate = xfrc_rate;
  n.max_samples = max_samples; n.max_horizon = max_horizon; n.device = device;
  p->Initialize(model, task, n);
  p->Allocate();
  return p;
}
void mjpc_robust_destroy(void* p) { delete (mjpc_hip::RobustPlanner*)p; }
void mjpc_robust_reset(void* p, int horizon) { ((mjpc_hip::RobustPlanner*)p)->Reset(horizon, nullptr); }
void mjpc_robust_set_state(void* p, const double* s, const double* m, const double* u, double t) { ((mjpc_hip::RobustPlanner*)p)->SetState(s, m, u, t); }
void mjpc_robust_set_seed(void* p, unsigned long long delegate_seed, unsigned long long robust_seed, unsigned long long plan_iter) {
  auto* q = (mjpc_hip::RobustPlanner*)p; q->delegate.seed = delegate_seed; q->delegate.plan_iter = plan_iter; q->seed = robust_seed; q->plan_iter = plan_iter;
}
void mjpc_robust_optimize_policy(void* p, int horizon) { ((mjpc_hip::RobustPlanner*)p)->OptimizePolicy(horizon); }
void mjpc_robust_action_from_policy(void* p, double* a, double t) { ((mjpc_hip::RobustPlanner*)p)->ActionFromPolicy(a, nullptr, t, false); }
// out[0] = best candidate, out[1] = candidates scored, out[2] = repetitions; scores[ncand], noisy_returns[ncand*rep] optional
void mjpc_robust_last(void* p, int* out, double* scores, double* noisy_returns) {
  auto* q = (mjpc_hip::RobustPlanner*)p;
  out[0] = q->best_candidate; out[1] = (int)q->candidate_scores.size(); out[2] = q->nrepetitions_;
  if (scores) std::copy(q->candidate_scores.begin(), q->candidate_scores.end(), scores);
  if (noisy_returns) std::copy(q->noisy_returns.begin(), q->noisy_returns.end(), noisy_returns);
}
void* mjpc_robust_delegate(void* p) { return &((mjpc_hip::RobustPlanner*)p)->delegate; }

}  // extern "C"

// ------------------------------------------------------------------ DirectCost
// The norms are the device's own functions (csrc/cost_derivatives.h: norm_grad_hess, norm_hess_entry), compiled for the host in a
// translation unit of their own (direct_norms.cc) the way the 1-lane emulation compiles them; everything around them is restated below.
namespace mjpc_hip {
namespace device_norms {
double norm_grad_hess(double* g, double* hd, double* hs, const double* x, const double* prm, int n, int type);
double norm_hess_entry(int type, const double* x, const double* g, const double* hs, int i, int j);
int norm_dense(int type);
}  // namespace device_norms

void DirectCost::Allocate(int nv, int nr, int T) {
  dim_v = nv; dim_residual = nr;
  noise_process.assign(nv, 1.0);
  SetSensors(0, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
  Size(T);
}

void DirectCost::SetSensors(int first_row, int num_sensor, const int* dim, const int* stage, const int* norm, const double* norm_parameter, const double* noise) {
  sensor_first_row = first_row;
  sensor_dim.assign(dim, dim + num_sensor); sensor_stage.assign(stage, stage + num_sensor); sensor_norm.assign(norm, norm + num_sensor);
  sensor_norm_parameter.assign(norm_parameter, norm_parameter + 2 * num_sensor); noise_sensor.assign(noise, noise + num_sensor);
  num_sensor_rows = std::accumulate(sensor_dim.begin(), sensor_dim.end(), 0);
  sensor_mask.clear();
}

void DirectCost::SetProcessNoise(const double* noise) { noise_process.assign(noise, noise + dim_v); }

void DirectCost::SetMask(const int* mask, int T) {
  if (mask) sensor_mask.assign(mask, mask + (size_t)T * sensor_dim.size()); else sensor_mask.clear();
}

void DirectCost::Size(int T) {
  const size_t Tz = T > 0 ? T : 0, nv = dim_v, ns = num_sensor_rows, nb = 3 * nv;
  gradient.assign(Tz * nv, 0.0); hessian_band.assign(Tz * nv * nb, 0.0);
  block_sensor.assign(Tz * ns * nb, 0.0); block_force.assign(Tz * nv * nb, 0.0);
  norm_gradient_sensor.assign(Tz * ns, 0.0); residual_sensor.assign(Tz * ns, 0.0);
  norm_gradient_force.assign(Tz * nv, 0.0); residual_force.assign(Tz * nv, 0.0);
  cost[0] = cost[1] = cost[2] = 0.0;
}

MjpcHipDirectSettings DirectCost::View(int T) const {
  MjpcHipDirectSettings s;
  std::memset(&s, 0, sizeof(s));
  s.struct_size = (int)sizeof(s);
  s.num_sensor = (int)sensor_dim.size(); s.sensor_first_row = sensor_first_row; s.num_sensor_rows = num_sensor_rows;
  s.sensor_dim = sensor_dim.data(); s.sensor_stage = sensor_stage.data(); s.sensor_norm = sensor_norm.data();
  s.sensor_norm_parameter = sensor_norm_parameter.data(); s.noise_sensor = noise_sensor.data(); s.noise_process = noise_process.data();
  s.sensor_mask = sensor_mask.empty() ? nullptr : sensor_mask.data();          // (the callers have checked that it covers T)
  s.sensor_flag = settings.sensor_flag; s.force_flag = settings.force_flag; s.time_scaling_sensor = settings.time_scaling_sensor;
  s.time_scaling_force = settings.time_scaling_force; s.first_step_position_sensors = settings.first_step_position_sensors;
  s.last_step_position_sensors = settings.last_step_position_sensors; s.last_step_velocity_sensors = settings.last_step_velocity_sensors;
  s.timestep = timestep;
  return s;
}

void DirectCost::SetWindow(int T, int nq, int na, int nu, const double* q, const double* a, const double* u, const double* time, const double* ys,
                           const double* yf) {
  window_length = T; dim_q = nq; dim_act = na; dim_action = nu;
  const size_t Tz = T > 0 ? T : 0;
  auto set = [](std::vector<double>& v, const double* src, size_t n) { if (src) v.assign(src, src + n); else v.assign(n, 0.0); };
  set(configuration, q, Tz * nq); set(act, a, Tz * na); set(ctrl, u, Tz * nu); set(times, time, Tz);
  set(sensor_measurement, ys, Tz * num_sensor_rows); set(force_measurement, yf, Tz * dim_v);
}

// a mask that does not cover the window is an error, not "every sensor on"
static bool MaskCovers(const std::vector<int>& mask, size_t T, size_t m) { return mask.empty() || mask.size() >= T * m; }

bool DirectCost::Cost(MjpcHipEngine* engine, const double* q_windows, int nwin, const double* mocap, const double* userdata) {
  const int T = window_length;
  if (!MaskCovers(sensor_mask, T, sensor_dim.size())) { Fatal("DirectCost: the mask holds fewer than T configurations"); return false; }
  if (!q_windows) { q_windows = configuration.data(); nwin = 1; }
  if (nwin < 1) { Fatal("DirectCost: nwin < 1"); return false; }
  const MjpcHipDirectSettings s = View(T);
  // act and ctrl are the window's for every candidate
  std::vector<double> a((size_t)nwin * act.size()), u((size_t)nwin * ctrl.size());
  for (int w = 0; w < nwin; w++) { std::copy(act.begin(), act.end(), a.begin() + w * act.size()); std::copy(ctrl.begin(), ctrl.end(), u.begin() + w * ctrl.size()); }
  costs.assign((size_t)3 * nwin, 0.0); failure.assign((size_t)nwin * (T > 0 ? T : 0), 0);
  const bool ok = mjpc_hip_direct_cost(engine, nwin, T, &s, discrete, q_windows, a.data(), u.data(), times.data(), sensor_measurement.data(),
                                       force_measurement.data(), mocap, userdata, costs.data(), nullptr, nullptr, nullptr, nullptr, failure.data()) == 0;
  if (ok) std::copy(costs.begin(), costs.begin() + 3, cost);
  return ok;
}

bool DirectCost::CostDerivatives(MjpcHipEngine* engine, const double* mocap, const double* userdata) {
  const int T = window_length;
  if (!MaskCovers(sensor_mask, T, sensor_dim.size())) { Fatal("DirectCost: the mask holds fewer than T configurations"); return false; }
  Size(T);
  failure.assign(T > 0 ? T : 0, 0);
  const MjpcHipDirectSettings s = View(T);
  auto p = [](std::vector<double>& v) { return v.empty() ? nullptr : v.data(); };
  return mjpc_hip_direct_cost_derivatives(engine, T, &s, fd_tolerance, fd_mode, discrete, configuration.data(), act.data(), ctrl.data(), times.data(),
                                          sensor_measurement.data(), force_measurement.data(), mocap, userdata, cost, p(gradient), p(hessian_band),
                                          p(block_sensor), p(block_force), p(norm_gradient_sensor), p(norm_gradient_force), p(residual_sensor),
                                          p(residual_force), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, failure.data()) == 0;
}

bool DirectCost::Assemble(MjpcHipEngine* engine, int T, const double* rs, const double* rf, const double* DfDq, const double* DfDv, const double* DfDa,
                          const double* DsDq, const double* DsDv, const double* DsDa, const double* dvdq0, const double* dvdq1) {
  if (!MaskCovers(sensor_mask, T > 0 ? T : 0, sensor_dim.size())) { Fatal("DirectCost: the mask holds fewer than T configurations"); return false; }
  Size(T);
  const MjpcHipDirectSettings s = View(T);
  auto p = [](std::vector<double>& v) { return v.empty() ? nullptr : v.data(); };
  return mjpc_hip_direct_assemble(engine, T, dim_v, dim_residual, &s, rs, rf, DfDq, DfDv, DfDa, DsDq, DsDv, DsDa, dvdq0, dvdq1, cost, p(gradient),
                                  p(hessian_band), p(block_sensor), p(block_force), p(norm_gradient_sensor), p(norm_gradient_force), p(residual_sensor),
                                  p(residual_force)) == 0;
}

// The order of mjpc_hip_direct_assemble (csrc/direct_cost.h), stage by stage over whole arrays: residuals, weights and norms; totals; the
// blocks J_t; N_t J_t; every gradient and band entry as its own sum.  Every product and every add below is rounded on its own.
bool DirectCost::AssembleHost(int T, const double* rs, const double* rf, const double* DfDq, const double* DfDv, const double* DfDa, const double* DsDq,
                              const double* DsDv, const double* DsDa, const double* dvdq0, const double* dvdq1) {
  const int nv = dim_v, nr = dim_residual, ns = num_sensor_rows, m = (int)sensor_dim.size(), nb = 3 * nv;
  if (T < 3) { Fatal("DirectCost: T < 3"); return false; }
  if (nv < 1) { Fatal("DirectCost: not allocated"); return false; }
  if (!(timestep > 0)) { Fatal("DirectCost: timestep <= 0"); return false; }
  if (sensor_first_row < 0 || sensor_first_row + ns > nr) { Fatal("DirectCost: the sensor rows lie outside the residual"); return false; }
  if (!MaskCovers(sensor_mask, T, sensor_dim.size())) { Fatal("DirectCost: the mask holds fewer than T configurations"); return false; }
  for (int i = 0; i < m; i++) {
    if (sensor_dim[i] < 1) { Fatal("DirectCost: a sensor dimension < 1"); return false; }
    if (sensor_stage[i] < 0 || sensor_stage[i] > 2) { Fatal("DirectCost: a sensor stage outside 0 .. 2"); return false; }
    if (!(noise_sensor[i] > 0)) { Fatal("DirectCost: a sensor noise value <= 0"); return false; }
  }
  for (int i = 0; i < nv; i++) if (!(noise_process[i] > 0)) { Fatal("DirectCost: a process noise value <= 0"); return false; }
  if ((ns && (!rs || !DsDq || !DsDv || !DsDa)) || !rf || !DfDq || !DfDv || !DfDa || !dvdq0 || !dvdq1) { Fatal("DirectCost: null input"); return false; }
  Size(T);
  const MjpcHipDirectSettings s = View(T);
  const double h = timestep, h2 = h * h, h4 = h2 * h2, ih = 1.0 / h;
  std::vector<int> first(m), owner(ns);
  for (int i = 0, r = 0; i < m; r += sensor_dim[i], i++) { first[i] = r; for (int k = 0; k < sensor_dim[i]; k++) owner[r + k] = i; }
  auto interior = [&](int t) { return t >= 1 && t <= T - 2; };
  auto masked = [&](int t, int i) { return s.sensor_mask && !s.sensor_mask[(size_t)t * m + i]; };
  std::vector<double> wf(nv);
  for (int i = 0; i < nv; i++) wf[i] = (settings.time_scaling_force ? h4 : 1.0) / noise_process[i] / (double)nv / (double)(T - 2);

  // residuals, weights, norms
  std::vector<double> hd((size_t)T * ns), hs((size_t)2 * T * m), w((size_t)T * m), yf(T, 0.0);
  double cs = 0.0, cf = 0.0;
  for (int t = 0; t < T; t++) {
    for (int i = 0; i < m; i++) {
      const int st = sensor_stage[i], n = sensor_dim[i];
      const bool keep = t == 0 ? st == kStagePos
                               : (t == T - 1 ? (st == kStagePos && settings.last_step_position_sensors) || (st == kStageVel && settings.last_step_velocity_sensors) : true);
      const size_t o = (size_t)t * ns + first[i], k = (size_t)t * m + i;
      double* x = residual_sensor.data() + o;
      for (int r = 0; r < n; r++) x[r] = keep ? rs[o + r] : 0.0;
      const double* prm = sensor_norm_parameter.data() + 2 * i;
      double y = device_norms::norm_grad_hess(norm_gradient_sensor.data() + o, hd.data() + o, hs.data() + 2 * k, x, prm, n, sensor_norm[i]);
      // the values that need no more than sqrt, by the summation rule
      double c = 0.0;
      switch (sensor_norm[i]) {
        case -1: y = x[0]; break;
        case 0: for (int r = 0; r < n; r++) c = c + x[r] * x[r]; y = 0.5 * c; break;
        case 2: for (int r = 0; r < n; r++) c = c + x[r] * x[r]; y = std::sqrt(c + prm[0] * prm[0]) + -prm[0]; break;
        case 6: for (int r = 0; r < n; r++) c = c + (std::sqrt(x[r] * x[r] + prm[0] * prm[0]) + -prm[0]); y = c; break;
        default: break;
      }
      double tw = 1.0;
      if (settings.time_scaling_sensor) tw = st == kStageVel ? h2 : (st == kStageAcc ? h4 : 1.0);
      double wi = tw / noise_sensor[i] / (double)n / (double)T;
      if (t == 0) wi = wi * (settings.first_step_position_sensors ? 1.0 : 0.0);
      if (t == T - 1) wi = wi * ((settings.last_step_position_sensors || settings.last_step_velocity_sensors) ? 1.0 : 0.0);
      w[k] = wi;
      if (settings.sensor_flag) cs = cs + (masked(t, i) ? 0.0 : wi * y);
    }
    for (int i = 0; i < nv; i++) {
      const size_t o = (size_t)t * nv + i;
      residual_force[o] = interior(t) ? rf[o] : 0.0;
      norm_gradient_force[o] = interior(t) ? wf[i] * rf[o] : 0.0;
    }
    if (interior(t)) {
      double c = 0.0;
      for (int i = 0; i < nv; i++) { const double r = rf[(size_t)t * nv + i]; c = c + r * (wf[i] * r); }
      yf[t] = 0.5 * c;
    }
  }
  if (settings.force_flag) for (int t = 1; t <= T - 2; t++) cf = cf + yf[t];
  cost[0] = cs + cf; cost[1] = cs; cost[2] = cf;

  // the blocks: row o < ns a sensor row, else dof o - ns of the force; (base + P1) + P2
  const double* Df[3] = {DfDq, DfDv, DfDa};
  const double* Ds[3] = {DsDq, DsDv, DsDa};
  auto D = [&](int t, int which, int o, int k) {
    if (o < ns) {
      const int st = sensor_stage[owner[o]];
      const bool keep = t == 0 ? (which == 0 && st == kStagePos) : (t == T - 1 ? (which < 2 && st < kStageAcc) : true);
      return keep ? Ds[which][((size_t)t * nr + sensor_first_row + o) * nv + k] : 0.0;
    }
    return interior(t) ? Df[which][((size_t)t * nv + (o - ns)) * nv + k] : 0.0;
  };
  auto J = [&](int t, int o, int c) -> double& {
    return o < ns ? block_sensor[((size_t)t * ns + o) * nb + c] : block_force[((size_t)t * nv + (o - ns)) * nb + c];
  };
  for (int t = 0; t < T; t++)
    for (int o = 0; o < ns + nv; o++)
      for (int c = 0; c < nb; c++) {
        const int g = c / nv, j = c % nv;
        const bool hasV = t >= 1 && g < 2, hasA = interior(t);
        double p1 = 0.0, p2 = 0.0;
        if (hasV) {
          const double* V = (g == 0 ? dvdq0 : dvdq1) + (size_t)t * nv * nv;
          for (int k = 0; k < nv; k++) p1 = p1 + D(t, 1, o, k) * V[(size_t)k * nv + j];
        }
        if (hasA)
          for (int k = 0; k < nv; k++) {
            const size_t e = ((size_t)t * nv + k) * nv + j, e1 = e + (size_t)nv * nv;
            const double A = g == 0 ? dvdq0[e] * -ih : (g == 1 ? (dvdq0[e1] + -dvdq1[e]) * ih : dvdq1[e1] * ih);
            p2 = p2 + D(t, 2, o, k) * A;
          }
        J(t, o, c) = ((g == 1 ? D(t, 0, o, j) : 0.0) + p1) + p2;
      }

  // N J
  std::vector<double> NJs((size_t)T * ns * nb), NJf((size_t)T * nv * nb);
  for (int t = 0; t < T; t++) {
    const size_t row = (size_t)t * ns;
    for (int o = 0; o < ns; o++) {
      const int i = owner[o], f = first[i], n = sensor_dim[i];
      for (int c = 0; c < nb; c++) {
        double v;
        if (!device_norms::norm_dense(sensor_norm[i])) v = hd[row + o] * block_sensor[(row + o) * nb + c];
        else {
          v = 0.0;
          for (int q = 0; q < n; q++)
            v = v + device_norms::norm_hess_entry(sensor_norm[i], residual_sensor.data() + row + f, norm_gradient_sensor.data() + row + f,
                                                  hs.data() + 2 * ((size_t)t * m + i), o - f, q) * block_sensor[(row + f + q) * nb + c];
        }
        NJs[(row + o) * nb + c] = v;
      }
    }
    for (int o = 0; o < nv; o++)
      for (int c = 0; c < nb; c++) { const size_t at = ((size_t)t * nv + o) * nb + c; NJf[at] = interior(t) ? wf[o] * block_force[at] : 0.0; }
  }

  // gradient and band: one sum per entry
  auto col = [&](int t, int G) {
    const int c = G - nv * (t - 1);
    if (c < 0 || c >= nb) return -1;
    if ((t == 0 && c / nv != 1) || (t == T - 1 && c / nv == 2)) return -1;
    return c;
  };
  auto sensor_sum = [&](int t, int ca, const double* X, int cb, double acc) {
    for (int i = 0; i < m; i++) {
      if (masked(t, i)) continue;
      const size_t row = (size_t)t * ns + first[i];
      double sum = 0.0;
      for (int r = 0; r < sensor_dim[i]; r++) sum = sum + block_sensor[(row + r) * nb + ca] * (X ? X[(row + r) * nb + cb] : norm_gradient_sensor[row + r]);
      acc = acc + w[(size_t)t * m + i] * sum;
    }
    return acc;
  };
  auto force_sum = [&](int t, int ca, const double* X, int cb, double acc) {
    const size_t row = (size_t)t * nv;
    double sum = 0.0;
    for (int r = 0; r < nv; r++) sum = sum + block_force[(row + r) * nb + ca] * (X ? X[(row + r) * nb + cb] : norm_gradient_force[row + r]);
    return acc + sum;
  };
  for (int R = 0; R < nv * T; R++) {
    const int lo = std::max(0, R / nv - 1), hi = std::min(T - 1, R / nv + 1);
    for (int C = 0; C <= nb; C++) {
      const int G = C == nb ? R : R - (nb - 1 - C);
      double es = 0.0, ef = 0.0;
      if (G >= 0)
        for (int t = lo; t <= hi; t++) {
          const int ca = col(t, R), cb = col(t, G);
          if (ca < 0 || cb < 0) continue;
          if (settings.sensor_flag) es = sensor_sum(t, ca, C == nb ? nullptr : NJs.data(), cb, es);
          if (settings.force_flag && interior(t)) ef = force_sum(t, ca, C == nb ? nullptr : NJf.data(), cb, ef);
        }
      (C == nb ? gradient[R] : hessian_band[(size_t)R * nb + C]) = es + ef;
    }
  }
  return true;
}

}  // namespace mjpc_hip

// ---- DirectCost
extern "C" {
void* mjpc_dc_create(int nv, int nr, int T) { auto* d = new mjpc_hip::DirectCost(); d->Allocate(nv, nr, T); return d; }
void mjpc_dc_destroy(void* dc) { delete (mjpc_hip::DirectCost*)dc; }
void mjpc_dc_set_sensors(void* dc, int first_row, int num_sensor, const int* dim, const int* stage, const int* norm, const double* norm_parameter,
                         const double* noise) {
  ((mjpc_hip::DirectCost*)dc)->SetSensors(first_row, num_sensor, dim, stage, norm, norm_parameter, noise);
}
void mjpc_dc_set_process_noise(void* dc, const double* noise) { ((mjpc_hip::DirectCost*)dc)->SetProcessNoise(noise); }
void mjpc_dc_set_mask(void* dc, const int* mask, int T) { ((mjpc_hip::DirectCost*)dc)->SetMask(mask, T); }
void mjpc_dc_set_settings(void* dc, const int* flags, double timestep) {
  auto* d = (mjpc_hip::DirectCost*)dc;
  d->settings.sensor_flag = flags[0]; d->settings.force_flag = flags[1]; d->settings.time_scaling_sensor = flags[2]; d->settings.time_scaling_force = flags[3];
  d->settings.first_step_position_sensors = flags[4]; d->settings.last_step_position_sensors = flags[5]; d->settings.last_step_velocity_sensors = flags[6];
  d->timestep = timestep;
}
int mjpc_dc_assemble(void* dc, MjpcHipEngine* engine, int T, const double* residual_sensor, const double* residual_force, const double* DfDq,
                     const double* DfDv, const double* DfDa, const double* DsDq, const double* DsDv, const double* DsDa, const double* dvdq0,
                     const double* dvdq1) {
  auto* d = (mjpc_hip::DirectCost*)dc;
  const bool ok = engine ? d->Assemble(engine, T, residual_sensor, residual_force, DfDq, DfDv, DfDa, DsDq, DsDv, DsDa, dvdq0, dvdq1)
                         : d->AssembleHost(T, residual_sensor, residual_force, DfDq, DfDv, DfDa, DsDq, DsDv, DsDa, dvdq0, dvdq1);
  return ok ? 0 : -1;
}
void mjpc_dc_set_window(void* dc, int T, int nq, int na, int nu, const double* q, const double* act, const double* ctrl, const double* time,
                        const double* sensor_measurement, const double* force_measurement) {
  ((mjpc_hip::DirectCost*)dc)->SetWindow(T, nq, na, nu, q, act, ctrl, time, sensor_measurement, force_measurement);
}
void mjpc_dc_set_fd(void* dc, double tolerance, int mode, int discrete) {
  auto* d = (mjpc_hip::DirectCost*)dc; d->fd_tolerance = tolerance; d->fd_mode = mode; d->discrete = discrete;
}
int mjpc_dc_cost(void* dc, MjpcHipEngine* engine, const double* q_windows, int nwin, const double* mocap, const double* userdata, double* costs, int* failure) {
  auto* d = (mjpc_hip::DirectCost*)dc;
  if (!d->Cost(engine, q_windows, nwin, mocap, userdata)) return -1;
  if (costs) std::copy(d->costs.begin(), d->costs.end(), costs);
  if (failure) std::copy(d->failure.begin(), d->failure.end(), failure);
  return 0;
}
int mjpc_dc_cost_derivatives(void* dc, MjpcHipEngine* engine, const double* mocap, const double* userdata, int* failure) {
  auto* d = (mjpc_hip::DirectCost*)dc;
  if (!d->CostDerivatives(engine, mocap, userdata)) return -1;
  if (failure) std::copy(d->failure.begin(), d->failure.end(), failure);
  return 0;
}
void mjpc_dc_outputs(void* dc, double* cost, double* gradient, double* hessian_band, double* block_sensor, double* block_force,
                     double* norm_gradient_sensor, double* norm_gradient_force, double* residual_sensor, double* residual_force) {
  auto* d = (mjpc_hip::DirectCost*)dc;
  if (cost) std::copy(d->cost, d->cost + 3, cost);
  double* out[8] = {gradient, hessian_band, block_sensor, block_force, norm_gradient_sensor, norm_gradient_force, residual_sensor, residual_force};
  const std::vector<double>* src[8] = {&d->gradient, &d->hessian_band, &d->block_sensor, &d->block_force, &d->norm_gradient_sensor,
                                       &d->norm_gradient_force, &d->residual_sensor, &d->residual_force};
  for (int k = 0; k < 8; k++) if (out[k]) std::copy(src[k]->begin(), src[k]->end(), out[k]);
}
}  // extern "C"
