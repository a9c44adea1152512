"""State estimators on the one-step engine: ctypes views of mjpc_hip::Kalman and mjpc_hip::Unscented (include/mjpc_hip_planner.h
via include/mjpc_hip_planner_c.h; the reference's mjpc/estimators/kalman.cc and unscented.cc).

    task = ResidualTable(model).sum(...).measurement()      # rows that are only sensors (or any task: pick the rows)
    be = HipBackend(model, task, max_samples=2 * nd + 1, max_horizon=2)
    ukf = Unscented(be)                                     # measurement = every residual row
    ukf.Reset(state, time)
    status = ukf.Update(ctrl, sensor)                       # 0, or an EstimatorStatus with the estimate untouched

The filter algebra runs in the C++ classes on the host, the model evaluations on the device (one mjpc_hip_linearize_step per EKF
half-step, one mjpc_hip_unscented_moments per UKF update).  There is no Python fall-back: a missing library raises in
capi.load_engine().  The pure functions at the bottom are the same algebra over numpy arrays, without an engine.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi

c_double_p = C.POINTER(C.c_double)
c_int_p = C.POINTER(C.c_int)

OK, COVARIANCE_RANK, SENSOR_RANK, STEP_FLAGGED, ENGINE_ERROR = range(5)      # mjpc_hip::EstimatorStatus

ESTIMATOR_C_SYMBOLS = [
    "mjpc_kalman_create", "mjpc_kalman_destroy", "mjpc_kalman_update_measurement", "mjpc_kalman_update_prediction", "mjpc_kalman_update",
    "mjpc_unscented_create", "mjpc_unscented_destroy", "mjpc_unscented_update", "mjpc_unscented_weights",
    "mjpc_estimator_reset", "mjpc_estimator_set_shared", "mjpc_estimator_dims", "mjpc_estimator_time", "mjpc_estimator_access",
    "mjpc_estimator_covariance_factor", "mjpc_estimator_kalman_gain", "mjpc_estimator_kalman_correct", "mjpc_estimator_covariance_predict",
    "mjpc_estimator_unscented_correct",
]

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    L = capi.load_engine()
    vp, d, i = C.c_void_p, C.c_double, C.c_int
    create = (vp, [vp, C.POINTER(capi.MjpcHipModel), C.POINTER(capi.MjpcHipTask), i, i, c_double_p])
    sig = {
        "mjpc_kalman_create": create, "mjpc_kalman_destroy": (None, [vp]),
        "mjpc_kalman_update_measurement": (i, [vp, c_double_p, c_double_p]), "mjpc_kalman_update_prediction": (i, [vp]),
        "mjpc_kalman_update": (i, [vp, c_double_p, c_double_p]),
        "mjpc_unscented_create": create, "mjpc_unscented_destroy": (None, [vp]),
        "mjpc_unscented_update": (i, [vp, c_double_p, c_double_p]), "mjpc_unscented_weights": (None, [vp, c_double_p]),
        "mjpc_estimator_reset": (None, [vp, c_double_p, d]), "mjpc_estimator_set_shared": (None, [vp, c_double_p, c_double_p]),
        "mjpc_estimator_dims": (None, [vp, c_int_p]), "mjpc_estimator_time": (d, [vp, c_double_p]),
        "mjpc_estimator_access": (None, [vp, i, c_double_p, c_double_p]),
        "mjpc_estimator_covariance_factor": (i, [i, c_double_p, c_double_p]),
        "mjpc_estimator_kalman_gain": (i, [i, i] + [c_double_p] * 6),
        "mjpc_estimator_kalman_correct": (None, [i, i] + [c_double_p] * 6),
        "mjpc_estimator_covariance_predict": (None, [i] + [c_double_p] * 3),
        "mjpc_estimator_unscented_correct": (i, [i, i] + [c_double_p] * 6),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res; f.argtypes = args
    _lib = L
    return L


def _in(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a if a.size else np.zeros(1)


def _dp(a):
    return None if a is None else a.ctypes.data_as(c_double_p)


def settings(epsilon=1.0e-6, flg_centered=False, alpha=1.0, beta=2.0, covariance_initial_scale=1.0e-4, process_noise_scale=1.0e-4,
             sensor_noise_scale=1.0e-4):
    """mjpc_hip::EstimatorSettings as the C view takes it"""
    return np.array([epsilon, 1.0 if flg_centered else 0.0, alpha, beta, covariance_initial_scale, process_noise_scale, sensor_noise_scale], float)


class _Estimator:
    """what Kalman and Unscented share: the estimate (state, covariance, time), the noises, Reset"""
    _create = _destroy = None

    def __init__(self, backend, sensor_first_row=0, num_sensor=None, **kw):
        self._L = lib()
        self.backend = backend            # keeps the engine alive: it is the caller's, the estimator only uses it
        nr = int(backend.task["num_residual"])
        ns = nr - int(sensor_first_row) if num_sensor is None else int(num_sensor)
        self._settings = settings(**kw)
        h = getattr(self._L, self._create)(backend.h, C.byref(backend.cm.c_model), C.byref(backend.cm.c_task), int(sensor_first_row), ns,
                                           _dp(self._settings))
        if not h:
            raise ValueError(f"sensor rows [{sensor_first_row}, {int(sensor_first_row) + ns}) are not inside the task's {nr} residual rows")
        self._handle = C.c_void_p(h)
        dims = np.zeros(4, np.int32)
        self._L.mjpc_estimator_dims(self._h, dims.ctypes.data_as(c_int_p))
        self.dim_state, self.dim_state_derivative, self.num_sensor = int(dims[0]), int(dims[1]), int(dims[2])

    @property
    def _h(self):
        """the C++ object; a closed estimator raises instead of handing NULL to the library"""
        h = getattr(self, "_handle", None)
        if not h:
            raise RuntimeError("the estimator is closed")
        return h

    def close(self):
        if getattr(self, "_handle", None):
            getattr(self._L, self._destroy)(self._handle); self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def Reset(self, state, time=0.0):
        """covariance = scale I, the noises filled with their scales (1e-4 by default, as in the reference)"""
        self._L.mjpc_estimator_reset(self._h, _dp(_in(state, self.dim_state)), float(time))

    def SetShared(self, mocap=None, userdata=None):
        self._L.mjpc_estimator_set_shared(self._h, None if mocap is None else _dp(_in(mocap)), None if userdata is None else _dp(_in(userdata)))

    def _access(self, which, shape, value=None):
        out = np.zeros(shape)
        self._L.mjpc_estimator_access(self._h, which, None if value is None else _dp(_in(value, shape)), _dp(out) if out.size else None)
        return out

    state = property(lambda s: s._access(0, s.dim_state), lambda s, v: s._access(0, s.dim_state, v))
    covariance = property(lambda s: s._access(1, (s.dim_state_derivative,) * 2), lambda s, v: s._access(1, (s.dim_state_derivative,) * 2, v))
    noise_process = property(lambda s: s._access(2, s.dim_state_derivative), lambda s, v: s._access(2, s.dim_state_derivative, v))
    noise_sensor = property(lambda s: s._access(3, s.num_sensor), lambda s, v: s._access(3, s.num_sensor, v))

    @property
    def time(self):
        return float(self._L.mjpc_estimator_time(self._h, None))

    @time.setter
    def time(self, t):
        self._L.mjpc_estimator_time(self._h, C.byref(C.c_double(float(t))))

    @property
    def last_failure(self):
        """the engine's MJPC_WARN_* bits of the last update"""
        dims = np.zeros(4, np.int32)
        self._L.mjpc_estimator_dims(self._h, dims.ctypes.data_as(c_int_p))
        return int(dims[3])

    def _io(self, ctrl, sensor):
        nu = self.backend.model["nu"]
        return _dp(_in(ctrl, nu) if nu else np.zeros(1)), _dp(_in(sensor, self.num_sensor))


class Kalman(_Estimator):
    """mjpc_hip::Kalman: an extended Kalman filter (kalman.cc:188-330).  Keyword settings: epsilon, flg_centered and the three scales."""
    _create, _destroy = "mjpc_kalman_create", "mjpc_kalman_destroy"

    def UpdateMeasurement(self, ctrl, sensor):
        return self._L.mjpc_kalman_update_measurement(self._h, *self._io(ctrl, sensor))

    def UpdatePrediction(self):
        return self._L.mjpc_kalman_update_prediction(self._h)

    def Update(self, ctrl, sensor):
        return self._L.mjpc_kalman_update(self._h, *self._io(ctrl, sensor))


class Unscented(_Estimator):
    """mjpc_hip::Unscented: an unscented Kalman filter (unscented.cc:484-574).  Keyword settings: alpha, beta and the three scales."""
    _create, _destroy = "mjpc_unscented_create", "mjpc_unscented_destroy"

    def Update(self, ctrl, sensor):
        return self._L.mjpc_unscented_update(self._h, *self._io(ctrl, sensor))

    @property
    def weights(self):
        """dict(sigma_step, weight_mean0, weight_covariance0, weight_sigma) (unscented.cc:134-143)"""
        w = np.zeros(4)
        self._L.mjpc_unscented_weights(self._h, _dp(w))
        return dict(sigma_step=w[0], weight_mean0=w[1], weight_covariance0=w[2], weight_sigma=w[3])


# ---- the filter algebra as pure functions (host, no GPU).  A status other than OK leaves the outputs as they were handed in.
def covariance_factor(P):
    """(status, L): the lower Cholesky factor of P"""
    P = _in(P); n = P.shape[0]
    Lf = np.full((n, n), np.nan)
    return lib().mjpc_estimator_covariance_factor(n, _dp(P), _dp(Lf)), Lf


def kalman_gain(P, Cm, R, fill=np.nan):
    """(status, PCt [nd, ns], factor [ns, ns] = chol(C P C' + diag R), gain [nd, ns])"""
    P = _in(P); Cm = _in(Cm); R = _in(R); nd, ns = P.shape[0], Cm.shape[0]
    PCt = np.full((nd, ns), fill); F = np.full((ns, ns), fill); G = np.full((nd, ns), fill)
    return lib().mjpc_estimator_kalman_gain(nd, ns, _dp(P), _dp(Cm), _dp(R), _dp(PCt), _dp(F), _dp(G)), PCt, F, G


def kalman_correct(PCt, factor, gain, sensor_error, P):
    """(correction [nd], P_new [nd, nd])"""
    PCt = _in(PCt); nd, ns = PCt.shape
    c = np.zeros(nd); Pn = np.array(_in(P, (nd, nd)), copy=True)
    lib().mjpc_estimator_kalman_correct(nd, ns, _dp(PCt), _dp(_in(factor)), _dp(_in(gain)), _dp(_in(sensor_error)), _dp(c), _dp(Pn))
    return c, Pn


def covariance_predict(A, Q, P):
    """sym(A P A' + diag Q)"""
    A = _in(A); nd = A.shape[0]
    Pn = np.array(_in(P, (nd, nd)), copy=True)
    lib().mjpc_estimator_covariance_predict(nd, _dp(A), _dp(_in(Q)), _dp(Pn))
    return Pn


def unscented_correct(cov_ss, cov_sy, cov_yy, sensor_error, fill=np.nan):
    """(status, correction [nd], P [nd, nd])"""
    cov_sy = _in(cov_sy); nd, ns = cov_sy.shape
    c = np.full(nd, fill); Pn = np.full((nd, nd), fill)
    rc = lib().mjpc_estimator_unscented_correct(nd, ns, _dp(_in(cov_ss)), _dp(cov_sy), _dp(_in(cov_yy)), _dp(_in(sensor_error)), _dp(c), _dp(Pn))
    return rc, c, Pn
