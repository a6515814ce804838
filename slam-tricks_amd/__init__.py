"""slam-tricks_amd -- MI355X-native nonlinear-least-squares / bundle-adjustment engine.

Python here is only a thin ctypes view of the C ABI (include/stba.h) exported by
slam-tricks_amd/libstba.so (HIP kernels for gfx950) plus the seeded scene generators; the
product is the shared library.  Nothing in this package imports, links or calls oracle/.
The library has no CPU fallback: on a machine without a HIP device every compute call raises
StbaError(STBA_ERR_NO_DEVICE).

Import with  importlib.import_module("slam-tricks_amd")  (the hyphen is the repository's name).
"""
import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("STBA_LIB") or os.path.join(_HERE, "libstba.so")   # STBA_LIB: kernel experiments only
TRACE_COLS = 7
TERM_REASON = {0: "none", 1: "gradient", 2: "function", 3: "parameter", 4: "max_iter",
               5: "min_radius", 6: "solver_fail", 7: "fixed", 8: "user"}
_lib = None


class StbaError(RuntimeError):
    def __init__(self, code, where):
        self.code = code
        msg = _lib.stba_last_error().decode() if _lib is not None else ""
        super().__init__(f"{where}: status {code} ({_lib.stba_status_string(code).decode()}) {msg}")


class LMOptions(C.Structure):
    _fields_ = [("max_num_iterations", C.c_int), ("initial_trust_region_radius", C.c_double),
                ("max_trust_region_radius", C.c_double), ("min_trust_region_radius", C.c_double),
                ("min_relative_decrease", C.c_double), ("min_lm_diagonal", C.c_double),
                ("max_lm_diagonal", C.c_double), ("function_tolerance", C.c_double),
                ("gradient_tolerance", C.c_double), ("parameter_tolerance", C.c_double),
                ("jacobi_scaling", C.c_int), ("num_threads", C.c_int),
                ("minimizer_progress_to_stdout", C.c_int), ("update_state_every_iteration", C.c_int),
                ("phase_timing", C.c_int), ("function_tolerance_takes_step", C.c_int)]


class LMSummary(C.Structure):
    _fields_ = [("termination_type", C.c_int), ("termination_reason", C.c_int), ("num_iterations", C.c_int),
                ("num_successful_steps", C.c_int), ("num_unsuccessful_steps", C.c_int),
                ("initial_cost", C.c_double), ("final_cost", C.c_double), ("final_radius", C.c_double),
                ("final_gradient_max_norm", C.c_double), ("seconds_total", C.c_double),
                ("ms_linearize", C.c_double), ("ms_schur", C.c_double), ("ms_solve", C.c_double),
                ("ms_backsub", C.c_double), ("ms_cost", C.c_double),
                ("ms_allreduce", C.c_double), ("allreduce_bytes", C.c_double), ("allreduce_calls", C.c_int)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["termination_reason"] = TERM_REASON.get(d["termination_reason"], "?")
        return d


ITER_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                      C.c_double, C.c_int)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
LINEARIZE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
RESIDUAL_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double))
PLUS_FN = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double))

# every symbol include/stba.h declares (tests check the library exports all of them)
EXPORTS = ["stba_status_string", "stba_last_error", "stba_version", "stba_device_count",
           "stba_lm_default_options", "stba_ba_create", "stba_ba_destroy", "stba_ba_set_params",
           "stba_ba_get_params", "stba_ba_set_schur_mode", "stba_ba_schur_mode", "stba_ba_set_host_linearizer", "stba_ba_set_allreduce", "stba_ba_reduced_dim", "stba_ba_evaluate",
           "stba_ba_cost", "stba_ba_normal_blocks", "stba_ba_reduced_system", "stba_ba_solve_reduced",
           "stba_ba_back_substitute", "stba_ba_apply_step", "stba_ba_solve", "stba_ba_lm_iterations",
           "stba_ba_triangulate", "stba_ba_time_linearize", "stba_ba_time_schur", "stba_cholesky_factor", "stba_cholesky_solve", "stba_cholesky_inverse",
           "stba_cholesky_time", "stba_cholesky_time_split", "stba_cholesky_schedule_model", "stba_cholesky_timeout_count", "stba_cholesky_set_timeout_us", "stba_cholesky_shard_model", "stba_cholesky_shard_owner", "stba_cholesky_profile", "stba_calib_evaluate", "stba_calib_gauss_newton",
           "stba_pcg_default_options", "stba_pg_create", "stba_pg_destroy", "stba_pg_set_allreduce", "stba_pg_get_poses", "stba_pg_evaluate",
           "stba_pg_solve", "stba_pg_last_pcg_summary", "stba_pg_time_kernels", "stba_dense_solve", "stba_corners_read", "stba_corners_write", "stba_zhang_init", "stba_two_view_init", "stba_odometry_read", "stba_odometry_write", "stba_trajectory_ate",
           "stba_comm_unique_id", "stba_comm_create", "stba_comm_destroy", "stba_comm_rank", "stba_comm_allreduce_sum",
           "stba_comm_allreduce_hook", "stba_ba_set_comm", "stba_pg_set_comm",
           "stba_ba_set_features", "stba_get_device", "stba_set_device",
           "stba_ba_covariance_compute", "stba_ba_camera_covariance", "stba_ba_point_covariance", "stba_ba_covariance_release",
           "stba_ba_camera_point_covariance", "stba_ba_point_pair_covariance",
           "stba_dense_covariance",
           "stba_ba_create_ex", "stba_ba_set_pcg", "stba_ba_last_pcg_summary", "stba_ba_schur_apply",
           "stba_ba_last_pcg_iterations", "stba_ba_time_schur_apply",
           "stba_ba_set_trust_region", "stba_ba_last_dogleg_summary",
           "stba_ba_set_inner_iterations", "stba_ba_inner_sweep", "stba_ba_last_inner_summary",
           "stba_pg_covariance_default_options", "stba_pg_covariance", "stba_pg_covariance_columns", "stba_pg_gauge_check",
           "stba_pg_set_information", "stba_pg_set_sqrt_information", "stba_pg_has_information",
           "stba_pg_set_loss", "stba_pg_has_loss",
           "stba_pg_set_priors", "stba_pg_prior_count", "stba_pg_evaluate_priors", "stba_pg_prior_kernel_geometry",
           "stba_ba_set_loss", "stba_ba_has_loss", "stba_ba_loss_kernel_geometry",
           "stba_ba_set_information", "stba_ba_set_sqrt_information", "stba_ba_has_information", "stba_ba_get_sqrt_information",
           "stba_ba_set_pose_priors", "stba_ba_pose_prior_count", "stba_ba_evaluate_pose_priors", "stba_ba_pose_prior_kernel_geometry",
           "stba_ba_set_relative_poses", "stba_ba_relative_pose_count", "stba_ba_evaluate_relative_poses",
           "stba_ba_relative_pose_kernel_geometry",
           "stba_ba_set_landmark_priors", "stba_ba_landmark_prior_count", "stba_ba_evaluate_landmark_priors",
           "stba_ba_landmark_prior_kernel_geometry",
           "stba_live_device_buffers"]


def lib():
    """Loads libstba.so; raises if it has not been built (no fallback of any kind)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run `python __graft_entry__.py build` "
                              "(hipcc, gfx950).  There is no CPU fallback.")
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.  If libstba (linked
        # against /opt/rocm) were loaded first and torch imported later, two runtimes would coexist
        # and torch.cuda would report "No HIP GPUs are available".  Importing torch first makes
        # libstba bind to the runtime torch already loaded (same soname).  Opt out with
        # STBA_NO_TORCH_PRELOAD=1 (pure C/C++ hosts never see this: they link /opt/rocm directly).
        if "torch" not in sys.modules and os.environ.get("STBA_NO_TORCH_PRELOAD", "0") != "1":
            try:
                import torch  # noqa: F401
            except Exception:
                pass
        L = C.CDLL(LIB_PATH)
        L.stba_status_string.restype = C.c_char_p
        L.stba_last_error.restype = C.c_char_p
        _lib = L
    return _lib


def _chk(code, where):
    if code != 0:
        raise StbaError(code, where)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def device_count():
    return lib().stba_device_count()


def live_device_buffers():
    """device buffers the library's engines, stores and calls hold right now (stba_live_device_buffers)"""
    n = C.c_longlong(0)
    _chk(lib().stba_live_device_buffers(C.byref(n)), "stba_live_device_buffers")
    return n.value


def default_options(**kw):
    o = LMOptions()
    lib().stba_lm_default_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


COMM_ID_BYTES = 128


def comm_unique_id():
    """rank 0: the 128-byte id every rank passes to Comm(...) (ncclGetUniqueId)"""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _chk(lib().stba_comm_unique_id(buf), "stba_comm_unique_id")
    return buf.raw


class Comm:
    """Native RCCL communicator (one per process / GPU): the engines all-reduce on their own stream through it,
    no Python on the data path."""

    def __init__(self, uid, rank, world, device=-1):
        self._h = C.c_void_p()
        self.rank, self.world = int(rank), int(world)
        _chk(lib().stba_comm_create(C.byref(self._h), C.c_char_p(bytes(uid)), self.rank, self.world, int(device)), "stba_comm_create")

    def allreduce_sum(self, ptr, count, stream=None):
        _chk(lib().stba_comm_allreduce_sum(self._h, C.c_void_p(ptr), C.c_size_t(count), C.c_void_p(stream or 0)),
             "stba_comm_allreduce_sum")

    def close(self):
        if self._h:
            lib().stba_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BACreateOptions(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("linear_solver", C.c_int)]


class DoglegSummary(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("factorizations", C.c_int), ("gauss_newton_solves", C.c_int), ("reused_steps", C.c_int),
                ("invalid_steps", C.c_int), ("steps_by_case", C.c_int * 3), ("final_mu", C.c_double)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "steps_by_case"}
        d["steps_by_case"] = list(self.steps_by_case)
        return d


INNER_MAX_GROUPS_REPORTED = 16


class InnerSummary(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("sweeps", C.c_int), ("disabled_at_iteration", C.c_int), ("sweep_ms", C.c_double),
                ("num_groups", C.c_int), ("group_size", C.c_int * INNER_MAX_GROUPS_REPORTED)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "group_size"}
        d["group_size"] = list(self.group_size)[: min(self.num_groups, INNER_MAX_GROUPS_REPORTED)]
        return d


def inner_ordering(n_cams, n_pts, tolerance=1e-3, rot_group=None, pos_group=None, pt_group=None):
    """checks the arguments of BAEngine.set_inner_iterations and returns (tolerance, rot, pos, pt) as the C ABI takes them (int32
    arrays or None).  Group ids are integers >= -1 (-1: not swept); all three None: the default ordering."""
    tol = float(tolerance)
    if not (np.isfinite(tol) and tol >= 0.0):
        raise ValueError(f"inner iteration tolerance must be finite and >= 0, not {tolerance!r}")
    out = []
    for name, g, n in (("rot_group", rot_group, n_cams), ("pos_group", pos_group, n_cams), ("pt_group", pt_group, n_pts)):
        if g is None:
            out.append(None)
            continue
        a = np.asarray(g)
        if a.shape != (n,):
            raise ValueError(f"{name} must have shape ({n},), not {a.shape}")
        if a.size and (not np.issubdtype(a.dtype, np.integer) or a.min() < -1):
            raise ValueError(f"{name} must hold integer group ids >= -1")
        out.append(np.ascontiguousarray(a, dtype=np.int32))
    return (tol, *out)


LINEAR_SOLVERS = {"dense_schur": 0, "iterative_schur": 1}
TRUST_REGIONS = {"lm": 0, "dogleg": 1}
PRECONDITIONERS = {"identity": 0, "jacobi": 1, "schur_jacobi": 2}


class BAEngine:
    """Device-resident bundle-adjustment problem (one landmark shard per engine).

    linear_solver: "dense_schur" (the reduced camera system formed and factored: stba_ba_create) or "iterative_schur" (PCG on the
    implicitly applied reduced system, no S: stba_ba_create_ex; set_pcg / pcg_summary / schur_apply)."""

    def __init__(self, cams, pts, obs_cam, obs_pt, obs_feat, cam_fixed=None, pt_fixed=None, stream=None, linear_solver="dense_schur",
                 loss=None, information=None, sqrt_information=None, pose_priors=None, relative_poses=None,
                 landmark_priors=None):
        """loss: per-observation robust losses as PGEngine takes them -- a kind name, a tuple (kind, a[, b[, scale]]) or a dict of
        set_loss's arguments.  information / sqrt_information (one of the two): per-observation 2 x 2 weights, the shapes that
        set_information takes.  pose_priors: dict(cams=, poses=, information= | sqrt_information=), set_pose_priors' arguments.
        relative_poses: dict(cam_i=, cam_j=, measurements=, information= | sqrt_information=), set_relative_poses' arguments.
        landmark_priors: dict(points=, positions=, information= | sqrt_information=), set_landmark_priors' arguments"""
        if information is not None and sqrt_information is not None:
            raise ValueError("BAEngine: give information or sqrt_information, not both")
        self._h = C.c_void_p()
        cams = _f64(cams).reshape(-1, 7)
        pts = _f64(pts).reshape(-1, 3)
        oc = np.ascontiguousarray(obs_cam, dtype=np.int32)
        op = np.ascontiguousarray(obs_pt, dtype=np.int32)
        of = _f64(obs_feat).reshape(-1, 2)
        cf = None if cam_fixed is None else np.ascontiguousarray(cam_fixed, dtype=np.uint8).reshape(-1, 6)
        pf = None if pt_fixed is None else np.ascontiguousarray(pt_fixed, dtype=np.uint8)
        self.nc, self.np_, self.no = len(cams), len(pts), len(oc)
        self._keep = []
        if linear_solver not in LINEAR_SOLVERS:
            raise ValueError(f"linear_solver must be one of {sorted(LINEAR_SOLVERS)}")
        self.linear_solver = linear_solver
        table = None if loss is None else self._loss_table(loss)
        weights = None
        if information is not None:
            weights = ("stba_ba_set_information", self._weight_array(information, "information"))
        elif sqrt_information is not None:
            weights = ("stba_ba_set_sqrt_information", self._weight_array(sqrt_information, "sqrt_information"))
        if linear_solver == "dense_schur":
            _chk(lib().stba_ba_create(C.byref(self._h), self.nc, self.np_, self.no, _p(cams), _p(pts), _p(oc), _p(op),
                                      _p(of), _p(cf), _p(pf), C.c_void_p(stream or 0)), "stba_ba_create")
        else:
            o = BACreateOptions(C.sizeof(BACreateOptions), LINEAR_SOLVERS[linear_solver])
            _chk(lib().stba_ba_create_ex(C.byref(self._h), self.nc, self.np_, self.no, _p(cams), _p(pts), _p(oc), _p(op),
                                         _p(of), _p(cf), _p(pf), C.c_void_p(stream or 0), C.byref(o)), "stba_ba_create_ex")
        if weights is not None:
            _chk(getattr(lib(), weights[0])(self._h, _p(weights[1])), weights[0])
        if table is not None:
            self._set_loss_table(table)
        if pose_priors is not None:
            self.set_pose_priors(**pose_priors)
        if relative_poses is not None:
            self.set_relative_poses(**relative_poses)
        if landmark_priors is not None:
            self.set_landmark_priors(**landmark_priors)

    def close(self):
        if self._h:
            lib().stba_ba_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- parameters
    def set_params(self, cams=None, pts=None):
        _chk(lib().stba_ba_set_params(self._h, _p(None if cams is None else _f64(cams)),
                                      _p(None if pts is None else _f64(pts))), "stba_ba_set_params")

    def set_features(self, obs_feat):
        """the observations' features again (n_obs x 2, the order given at creation): stba_ba_set_features"""
        f = _f64(obs_feat)
        assert f.size == 2 * self.no
        _chk(lib().stba_ba_set_features(self._h, _p(f)), "stba_ba_set_features")

    def get_params(self):
        cams = np.zeros((self.nc, 7)); pts = np.zeros((self.np_, 3))
        _chk(lib().stba_ba_get_params(self._h, _p(cams), _p(pts)), "stba_ba_get_params")
        return cams, pts

    # ---- robust losses
    def _loss_table(self, loss):
        kw = dict(who="BAEngine", what="observation")
        if isinstance(loss, dict):
            return pg_loss_table(self.no, **loss, **kw)
        if isinstance(loss, tuple):
            return pg_loss_table(self.no, *loss, **kw)
        return pg_loss_table(self.no, loss, **kw)

    def _set_loss_table(self, table):
        kind, a, b, scale = table
        _chk(lib().stba_ba_set_loss(self._h, _p(kind), _p(a), _p(b), _p(scale)), "stba_ba_set_loss")

    def set_loss(self, kind, a=None, b=None, scale=None):
        """robust losses (Ceres' kinds, LOSS_KINDS), per observation in the order given at creation: the cost becomes
        1/2 sum rho_i(|r_i|^2).  One spec for all observations -- set_loss("cauchy", 0.05) -- or sequences of length n_obs:
        set_loss(["huber", None, ...], a_array).  b is TolerantLoss' second parameter; scale multiplies the loss (ScaledLoss).
        evaluate() then returns the corrected r, Jc, Jp, covariance() (J'^T J')^-1 (include/stba.h).  set_loss(None): no loss, the
        engine as it was."""
        if kind is None and a is None and b is None and scale is None:
            _chk(lib().stba_ba_set_loss(self._h, None, None, None, None), "stba_ba_set_loss")
            return
        self._set_loss_table(pg_loss_table(self.no, kind, a, b, scale, who="BAEngine", what="observation"))

    @property
    def has_loss(self):
        has = C.c_int()
        _chk(lib().stba_ba_has_loss(self._h, C.byref(has)), "stba_ba_has_loss")
        return bool(has.value)

    # ---- per-observation information matrices
    def _weight_array(self, w, name):
        """(n_obs, 4) float64 from a (2, 2) for all observations, an (n_obs, 2, 2), or a scalar / an (n_obs,) array w_i meaning
        w_i * I (for the information form: g2o's invSigma2)"""
        w = np.asarray(w, np.float64)
        if w.ndim == 0:
            w = np.full(self.no, float(w))
        if w.ndim == 1:
            if w.shape != (self.no,):
                raise ValueError(f"BAEngine: per-observation {name} must be a number or have length {self.no}, got {w.shape}")
            out = np.zeros((self.no, 4))
            out[:, 0] = w
            out[:, 3] = w
            return out
        if w.shape == (2, 2):
            return np.ascontiguousarray(np.broadcast_to(w.reshape(1, 4), (self.no, 4)))
        if w.shape != (self.no, 2, 2):
            raise ValueError(f"BAEngine: per-observation {name} must have shape (2, 2) or ({self.no}, 2, 2), got {w.shape}")
        return np.ascontiguousarray(w.reshape(self.no, 4))

    def set_information(self, information):
        """per-observation 2 x 2 information matrices Omega_i (symmetric positive definite), in the order given at creation: the
        cost becomes 1/2 sum rho_i(r_i^T Omega_i r_i).  A (2, 2) for all observations, an (n_obs, 2, 2), or a scalar / an (n_obs,)
        array w_i meaning w_i * I.  evaluate() then returns the whitened r, Jc, Jp (W_i = L_i^T, Omega_i = L_i L_i^T), covariance()
        (J^T Omega J)^-1 (include/stba.h).  set_information(None), or weights that are all exactly the identity: no weights, the
        engine as it was (has_information is False)."""
        arr = None if information is None else self._weight_array(information, "information")
        _chk(lib().stba_ba_set_information(self._h, _p(arr)), "stba_ba_set_information")

    def set_sqrt_information(self, sqrt_information):
        """as set_information, from square-root information matrices W_i (any finite 2 x 2, Omega_i = W_i^T W_i); a scalar or an
        (n_obs,) array means w_i * I as W.  None: the identity."""
        arr = None if sqrt_information is None else self._weight_array(sqrt_information, "sqrt_information")
        _chk(lib().stba_ba_set_sqrt_information(self._h, _p(arr)), "stba_ba_set_sqrt_information")

    @property
    def has_information(self):
        has = C.c_int()
        _chk(lib().stba_ba_has_information(self._h, C.byref(has)), "stba_ba_has_information")
        return bool(has.value)

    def sqrt_information(self):
        """(n_obs, 2, 2): the W_i the engine holds, in the order given at creation (identities if it holds none)"""
        out = np.empty((self.no, 2, 2))
        _chk(lib().stba_ba_get_sqrt_information(self._h, _p(out)), "stba_ba_get_sqrt_information")
        return out

    # ---- camera pose priors
    def set_pose_priors(self, cams, poses, information=None, sqrt_information=None):
        """soft constraints on camera poses (stba_ba_set_pose_priors): prior k pulls camera cams[k] towards poses[k] = [qx, qy, qz, qw,
        tx, ty, tz] (camera to world, like the engine's cameras) with cost 1/2 |W_k r_k|^2, r_k = [Log(qh^-1 q); t - th] in the order
        [rot(3), pos(3)].  information: (n, 6, 6) symmetric positive definite (W = L^T of its Cholesky factor) or sqrt_information:
        (n, 6, 6) any finite W (zero rotation rows: a position-only prior); a single (6, 6) is taken for every prior; neither: the
        identity.  Several priors may name one camera.  cams empty (or None) clears the priors."""
        if information is not None and sqrt_information is not None:
            raise ValueError("BAEngine: give information or sqrt_information, not both")
        c = np.ascontiguousarray([] if cams is None else cams, dtype=np.int32).reshape(-1)
        n = len(c)
        if n == 0:
            _chk(lib().stba_ba_set_pose_priors(self._h, 0, None, None, None, None), "stba_ba_set_pose_priors")
            return
        ps = _f64(poses).reshape(-1, 7)
        if len(ps) != n:
            raise ValueError(f"BAEngine: {n} prior cameras but {len(ps)} prior poses")

        def blocks(w, name):
            if w is None:
                return None
            w = np.asarray(w, np.float64)
            if w.shape == (6, 6):
                w = np.broadcast_to(w, (n, 6, 6))
            if w.shape != (n, 6, 6):
                raise ValueError(f"BAEngine: pose-prior {name} must have shape (6, 6) or ({n}, 6, 6), got {w.shape}")
            return np.ascontiguousarray(w)
        om, w = blocks(information, "information"), blocks(sqrt_information, "sqrt_information")
        _chk(lib().stba_ba_set_pose_priors(self._h, n, _p(c), _p(ps), _p(om), _p(w)), "stba_ba_set_pose_priors")

    def pose_prior_count(self):
        n = C.c_int()
        _chk(lib().stba_ba_pose_prior_count(self._h, C.byref(n)), "stba_ba_pose_prior_count")
        return n.value

    def evaluate_pose_priors(self, jac=True):
        """(cost, r [n, 6], J [n, 6, 6] | None) of the priors alone at the current parameters: whitened, in the order they were set"""
        n = self.pose_prior_count()
        cost = C.c_double()
        r = np.zeros((n, 6))
        J = np.zeros((n, 6, 6)) if jac else None
        _chk(lib().stba_ba_evaluate_pose_priors(self._h, C.byref(cost), _p(r), _p(J)), "stba_ba_evaluate_pose_priors")
        return cost.value, r, J

    def pose_prior_kernel_geometry(self):
        """cameras with priors per workgroup of the block kernel (a diagnostic: stba_ba_pose_prior_kernel_geometry)"""
        k = C.c_int()
        _chk(lib().stba_ba_pose_prior_kernel_geometry(self._h, C.byref(k)), "stba_ba_pose_prior_kernel_geometry")
        return k.value

    # ---- camera-to-camera relative-pose factors
    def set_relative_poses(self, cam_i, cam_j, measurements, information=None, sqrt_information=None):
        """odometry / loop-closure edges between cameras (stba_ba_set_relative_poses): edge k says that camera cam_j[k], seen from camera
        cam_i[k], sits at measurements[k] = [qx, qy, qz, qw, tx, ty, tz], with cost 1/2 |W_k r_k|^2, r_k = [Log(qz^-1 q_i^-1 q_j);
        R_i^T (t_j - t_i) - tz] in the order [rot(3), pos(3)].  information / sqrt_information: the shapes set_pose_priors takes.
        Several edges may name one pair, in either direction.  cam_i empty (or None) clears the edges."""
        if information is not None and sqrt_information is not None:
            raise ValueError("BAEngine: give information or sqrt_information, not both")
        ci = np.ascontiguousarray([] if cam_i is None else cam_i, dtype=np.int32).reshape(-1)
        n = len(ci)
        if n == 0:
            _chk(lib().stba_ba_set_relative_poses(self._h, 0, None, None, None, None, None), "stba_ba_set_relative_poses")
            return
        cj = np.ascontiguousarray(cam_j, dtype=np.int32).reshape(-1)
        ms = _f64(measurements).reshape(-1, 7)
        if len(cj) != n or len(ms) != n:
            raise ValueError(f"BAEngine: {n} cam_i but {len(cj)} cam_j and {len(ms)} measurements")

        def blocks(w, name):
            if w is None:
                return None
            w = np.asarray(w, np.float64)
            if w.shape == (6, 6):
                w = np.broadcast_to(w, (n, 6, 6))
            if w.shape != (n, 6, 6):
                raise ValueError(f"BAEngine: relative-pose {name} must have shape (6, 6) or ({n}, 6, 6), got {w.shape}")
            return np.ascontiguousarray(w)
        om, w = blocks(information, "information"), blocks(sqrt_information, "sqrt_information")
        _chk(lib().stba_ba_set_relative_poses(self._h, n, _p(ci), _p(cj), _p(ms), _p(om), _p(w)), "stba_ba_set_relative_poses")

    def relative_pose_count(self):
        n = C.c_int()
        _chk(lib().stba_ba_relative_pose_count(self._h, C.byref(n)), "stba_ba_relative_pose_count")
        return n.value

    def evaluate_relative_poses(self, jac=True):
        """(cost, r [n, 6], Ji [n, 6, 6] | None, Jj [n, 6, 6] | None) of the edges alone at the current parameters: whitened, in the
        order they were set"""
        n = self.relative_pose_count()
        cost = C.c_double()
        r = np.zeros((n, 6))
        Ji = np.zeros((n, 6, 6)) if jac else None
        Jj = np.zeros((n, 6, 6)) if jac else None
        _chk(lib().stba_ba_evaluate_relative_poses(self._h, C.byref(cost), _p(r), _p(Ji), _p(Jj)), "stba_ba_evaluate_relative_poses")
        return cost.value, r, Ji, Jj

    def relative_pose_kernel_geometry(self):
        """groups (cameras with edges, then pairs with edges) per workgroup of the block kernel (a diagnostic)"""
        k = C.c_int()
        _chk(lib().stba_ba_relative_pose_kernel_geometry(self._h, C.byref(k)), "stba_ba_relative_pose_kernel_geometry")
        return k.value

    # ---- landmark position priors (control points)
    def set_landmark_priors(self, points, positions, information=None, sqrt_information=None):
        """soft constraints on landmark positions (stba_ba_set_landmark_priors): prior k pulls landmark points[k] towards positions[k]
        with cost 1/2 |W_k (p - positions[k])|^2 -- a ground control point, a map or LiDAR point, a depth prior.  information:
        (n, 3, 3) symmetric positive definite (W = L^T of its Cholesky factor) or sqrt_information: (n, 3, 3) any finite W (one
        non-zero row: a height-only control point); a single (3, 3) is taken for every prior, an (n,) array of sigmas means I / sigma;
        neither: the identity.  Several priors may name one landmark.  points empty (or None) clears the priors."""
        if information is not None and sqrt_information is not None:
            raise ValueError("BAEngine: give information or sqrt_information, not both")
        j = np.ascontiguousarray([] if points is None else points, dtype=np.int32).reshape(-1)
        n = len(j)
        if n == 0:
            _chk(lib().stba_ba_set_landmark_priors(self._h, 0, None, None, None, None), "stba_ba_set_landmark_priors")
            return
        ps = _f64(positions).reshape(-1, 3)
        if len(ps) != n:
            raise ValueError(f"BAEngine: {n} prior landmarks but {len(ps)} prior positions")

        def blocks(w, name, power):
            if w is None:
                return None
            w = np.asarray(w, np.float64)
            if w.shape == (n,):                     # sigmas
                w = (w ** power)[:, None, None] * np.eye(3)[None]
            if w.shape == (3, 3):
                w = np.broadcast_to(w, (n, 3, 3))
            if w.shape != (n, 3, 3):
                raise ValueError(f"BAEngine: landmark-prior {name} must have shape (3, 3), ({n}, 3, 3) or ({n},), got {w.shape}")
            return np.ascontiguousarray(w)
        om, w = blocks(information, "information", -2.0), blocks(sqrt_information, "sqrt_information", -1.0)
        _chk(lib().stba_ba_set_landmark_priors(self._h, n, _p(j), _p(ps), _p(om), _p(w)), "stba_ba_set_landmark_priors")

    def landmark_prior_count(self):
        n = C.c_int()
        _chk(lib().stba_ba_landmark_prior_count(self._h, C.byref(n)), "stba_ba_landmark_prior_count")
        return n.value

    def evaluate_landmark_priors(self, jac=True):
        """(cost, r [n, 3], J [n, 3, 3] | None) of the landmark priors alone at the current parameters: whitened, in the order they
        were set"""
        n = self.landmark_prior_count()
        cost = C.c_double()
        r = np.zeros((n, 3))
        J = np.zeros((n, 3, 3)) if jac else None
        _chk(lib().stba_ba_evaluate_landmark_priors(self._h, C.byref(cost), _p(r), _p(J)), "stba_ba_evaluate_landmark_priors")
        return cost.value, r, J

    def landmark_prior_kernel_geometry(self):
        """landmarks per workgroup of the block kernel (a diagnostic: stba_ba_landmark_prior_kernel_geometry)"""
        k = C.c_int()
        _chk(lib().stba_ba_landmark_prior_kernel_geometry(self._h, C.byref(k)), "stba_ba_landmark_prior_kernel_geometry")
        return k.value

    def loss_kernel_geometry(self):
        """(observations per workgroup tile of the correcting linearisation kernel, whether this engine's cameras are staged in its
        LDS, the largest camera count that still is): stba_ba_loss_kernel_geometry"""
        t, c, m = C.c_int(), C.c_int(), C.c_int()
        _chk(lib().stba_ba_loss_kernel_geometry(self._h, C.byref(t), C.byref(c), C.byref(m)), "stba_ba_loss_kernel_geometry")
        return t.value, bool(c.value), m.value

    def set_allreduce(self, fn, rank, world):
        cb = ALLREDUCE_FN(fn)
        self._keep.append(cb)
        _chk(lib().stba_ba_set_allreduce(self._h, cb, None, rank, world), "stba_ba_set_allreduce")

    def set_host_linearizer(self, fn):
        """fn(cams[nc,7], pts[np,3], want_jac) -> (r[no,2], Jc[no,2,6] | None, Jp[no,2,3] | None) in the CALLER's observation order
        (stba_ba_set_host_linearizer: the factors are evaluated on the host, everything behind them runs on the device)"""
        nc, np_, no = self.nc, self.np_, self.no

        def tramp(user, cams_p, pts_p, r_p, jc_p, jp_p):
            try:
                cams = np.ctypeslib.as_array(C.cast(cams_p, C.POINTER(C.c_double)), (nc, 7))
                pts = np.ctypeslib.as_array(C.cast(pts_p, C.POINTER(C.c_double)), (np_, 3))
                want = bool(jc_p)
                r, Jc, Jp = fn(cams, pts, want)
                np.ctypeslib.as_array(C.cast(r_p, C.POINTER(C.c_double)), (no, 2))[:] = r
                if want:
                    np.ctypeslib.as_array(C.cast(jc_p, C.POINTER(C.c_double)), (no, 2, 6))[:] = Jc
                    np.ctypeslib.as_array(C.cast(jp_p, C.POINTER(C.c_double)), (no, 2, 3))[:] = Jp
                return 0
            except Exception:
                return 1
        cb = LINEARIZE_FN(tramp)
        self._keep.append(cb)
        _chk(lib().stba_ba_set_host_linearizer(self._h, cb, None), "stba_ba_set_host_linearizer")

    def set_comm(self, comm):
        """landmark shard of a multi-GPU solve: cross-rank sums through a native RCCL communicator"""
        self._keep.append(comm)
        _chk(lib().stba_ba_set_comm(self._h, comm._h if comm is not None else None), "stba_ba_set_comm")

    def reduced_dim(self):
        n, npad = C.c_int(), C.c_int()
        _chk(lib().stba_ba_reduced_dim(self._h, C.byref(n), C.byref(npad)), "stba_ba_reduced_dim")
        return n.value, npad.value

    # ---- stages
    def evaluate(self, jac=True, residuals=True):
        cost = C.c_double()
        r = np.zeros((self.no, 2)) if residuals else None
        Jc = np.zeros((self.no, 2, 6)) if jac else None
        Jp = np.zeros((self.no, 2, 3)) if jac else None
        _chk(lib().stba_ba_evaluate(self._h, C.byref(cost), _p(r), _p(Jc), _p(Jp)), "stba_ba_evaluate")
        return cost.value, r, Jc, Jp

    def cost(self):
        c = C.c_double()
        _chk(lib().stba_ba_cost(self._h, C.byref(c)), "stba_ba_cost")
        return c.value

    def normal_blocks(self):
        Hcc = np.zeros((self.nc, 6, 6)); gc = np.zeros((self.nc, 6))
        Hpp = np.zeros((self.np_, 3, 3)); gp = np.zeros((self.np_, 3))
        _chk(lib().stba_ba_normal_blocks(self._h, _p(Hcc), _p(gc), _p(Hpp), _p(gp)), "stba_ba_normal_blocks")
        return Hcc, gc, Hpp, gp

    def reduced_system(self, dc, dp, fetch=True):
        n = 6 * self.nc
        S = np.zeros((n, n)) if fetch else None
        rhs = np.zeros(n) if fetch else None
        _chk(lib().stba_ba_reduced_system(self._h, _p(_f64(dc)), _p(_f64(dp)), _p(S), _p(rhs)),
             "stba_ba_reduced_system")
        return S, rhs

    def solve_reduced(self):
        dxc = np.zeros(6 * self.nc)
        _chk(lib().stba_ba_solve_reduced(self._h, _p(dxc)), "stba_ba_solve_reduced")
        return dxc

    def back_substitute(self):
        dxp = np.zeros((self.np_, 3))
        _chk(lib().stba_ba_back_substitute(self._h, _p(dxp)), "stba_ba_back_substitute")
        return dxp

    def apply_step(self, accept=True):
        c = C.c_double()
        _chk(lib().stba_ba_apply_step(self._h, int(bool(accept)), C.byref(c)), "stba_ba_apply_step")
        return c.value

    # ---- solves
    def solve(self, opt=None, callback=None, **kw):
        opt = opt or default_options(**kw)
        trace = np.zeros((opt.max_num_iterations + 1, TRACE_COLS))
        summ = LMSummary()
        cb = ITER_CB(callback) if callback else C.cast(None, ITER_CB)
        _chk(lib().stba_ba_solve(self._h, C.byref(opt), C.byref(summ), _p(trace), cb, None), "stba_ba_solve")
        return summ, trace[: summ.num_iterations + 1]

    def covariance(self, cam_pairs=None, points=None, min_rcond=1e-14):
        """covariance of the undamped problem at the current parameters (stba_ba_covariance_compute): returns
        (cam_blocks [k,6,6], point_blocks [m,3,3], rcond).  cam_pairs: (a, b) pairs, default every camera's diagonal block;
        points: landmark indices, default all.  Tangent coordinates [rot(3), pos(3)] per camera, 3 per landmark."""
        L = lib()
        rc = C.c_double()
        _chk(L.stba_ba_covariance_compute(self._h, C.c_double(min_rcond), C.byref(rc)), "stba_ba_covariance_compute")
        if cam_pairs is None:
            ca = cb = np.arange(self.nc, dtype=np.int32)
        else:
            pr = np.asarray(cam_pairs, dtype=np.int32).reshape(-1, 2)
            ca, cb = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
        cam = np.zeros((len(ca), 6, 6))
        _chk(L.stba_ba_camera_covariance(self._h, len(ca), _p(ca), _p(cb), _p(cam)), "stba_ba_camera_covariance")
        pts = None if points is None else np.ascontiguousarray(points, dtype=np.int32).reshape(-1)
        m = self.np_ if pts is None else len(pts)
        pb = np.zeros((m, 3, 3))
        _chk(L.stba_ba_point_covariance(self._h, m, _p(pts), _p(pb)), "stba_ba_point_covariance")
        return cam, pb, rc.value

    def cross_covariance(self, cam_points=(), point_pairs=(), min_rcond=1e-14, recompute=True):
        """off-diagonal blocks of the same covariance: returns (cp [k,6,3], pp [m,3,3], rcond).  cam_points: (camera, landmark)
        pairs -> Sigma[camera, landmark] (rows [rot(3), pos(3)]); point_pairs: (j, k) landmark pairs -> Sigma[j, k] ((j, j): the
        marginal covariance() gives; (k, j) is bitwise the transpose of (j, k)).  recompute=False takes the blocks from what the
        last covariance() or cross_covariance() left on the device (StbaError -6 if nothing is held); rcond is then None."""
        L = lib()
        rcond = None
        if recompute:
            rc = C.c_double()
            _chk(L.stba_ba_covariance_compute(self._h, C.c_double(min_rcond), C.byref(rc)), "stba_ba_covariance_compute")
            rcond = rc.value
        cpr = np.asarray(cam_points, dtype=np.int32).reshape(-1, 2)
        ca, pj = np.ascontiguousarray(cpr[:, 0]), np.ascontiguousarray(cpr[:, 1])
        cp = np.zeros((len(ca), 6, 3))
        _chk(L.stba_ba_camera_point_covariance(self._h, len(ca), _p(ca), _p(pj), _p(cp)), "stba_ba_camera_point_covariance")
        ppr = np.asarray(point_pairs, dtype=np.int32).reshape(-1, 2)
        pa, pb = np.ascontiguousarray(ppr[:, 0]), np.ascontiguousarray(ppr[:, 1])
        pp = np.zeros((len(pa), 3, 3))
        _chk(L.stba_ba_point_pair_covariance(self._h, len(pa), _p(pa), _p(pb), _p(pp)), "stba_ba_point_pair_covariance")
        return cp, pp, rcond

    def covariance_release(self):
        _chk(lib().stba_ba_covariance_release(self._h), "stba_ba_covariance_release")

    def lm_iterations(self, iterations, opt=None, **kw):
        opt = opt or default_options(**kw)
        trace = np.zeros((iterations + 1, TRACE_COLS))
        summ = LMSummary()
        _chk(lib().stba_ba_lm_iterations(self._h, C.byref(opt), int(iterations), C.byref(summ), _p(trace)),
             "stba_ba_lm_iterations")
        return summ, trace

    def triangulate(self, max_iter=50):
        _chk(lib().stba_ba_triangulate(self._h, int(max_iter)), "stba_ba_triangulate")

    def time_linearize(self, reps=20):
        ms = C.c_double()
        _chk(lib().stba_ba_time_linearize(self._h, int(reps), C.byref(ms)), "stba_ba_time_linearize")
        return ms.value

    SCHUR_AUTO, SCHUR_PAIRS, SCHUR_DENSE = 0, 1, 2

    def set_schur_mode(self, mode):
        """form of the Schur complement: SCHUR_PAIRS (pair plan, LDS accumulation) | SCHUR_DENSE (S = -(Y Y^T) on the matrix cores,
        for dense visibility) | SCHUR_AUTO (what the engine chose at creation)"""
        _chk(lib().stba_ba_set_schur_mode(self._h, int(mode)), "stba_ba_set_schur_mode")

    def schur_mode(self):
        m = C.c_int()
        _chk(lib().stba_ba_schur_mode(self._h, C.byref(m)), "stba_ba_schur_mode")
        return m.value

    # ---- iterative Schur
    def set_pcg(self, preconditioner="jacobi", eta=0.1, min_iterations=0, max_iterations=500, check_every=4):
        """PCG of an "iterative_schur" engine (Ceres' defaults): preconditioner identity | jacobi | schur_jacobi, eta = q_tolerance"""
        pc = PRECONDITIONERS[preconditioner] if isinstance(preconditioner, str) else int(preconditioner)
        _chk(lib().stba_ba_set_pcg(self._h, pc, C.c_double(eta), int(min_iterations), int(max_iterations), int(check_every)),
             "stba_ba_set_pcg")

    def pcg_summary(self):
        s = PCGSummary()
        _chk(lib().stba_ba_last_pcg_summary(self._h, C.byref(s)), "stba_ba_last_pcg_summary")
        return s

    def pcg_iterations(self, n):
        """PCG iterations of LM iterations 1 .. n of the last solve (stba_ba_last_pcg_iterations)"""
        out = np.zeros(int(n), dtype=np.int32)
        _chk(lib().stba_ba_last_pcg_iterations(self._h, _p(out), int(n)), "stba_ba_last_pcg_iterations")
        return out

    # ---- trust-region strategy
    def set_trust_region(self, strategy):
        """"lm" (Levenberg-Marquardt, the default) | "dogleg" (Powell's dogleg, Ceres' TRADITIONAL_DOGLEG): what solve() runs
        (stba_ba_set_trust_region; lm_iterations always runs LM).  DOGLEG needs the dense Schur solver and one rank."""
        if isinstance(strategy, str) and strategy not in TRUST_REGIONS:
            raise ValueError(f"trust region strategy must be one of {sorted(TRUST_REGIONS)}, not {strategy!r}")
        code = TRUST_REGIONS[strategy] if isinstance(strategy, str) else int(strategy)
        _chk(lib().stba_ba_set_trust_region(self._h, code), "stba_ba_set_trust_region")

    def dogleg_summary(self):
        """factorisations, Gauss-Newton solves, re-used and invalid steps, steps per case and the final mu of the last solve"""
        s = DoglegSummary()
        s.struct_size = C.sizeof(DoglegSummary)
        _chk(lib().stba_ba_last_dogleg_summary(self._h, C.byref(s)), "stba_ba_last_dogleg_summary")
        return s

    # ---- inner iterations (Ceres' use_inner_iterations; include/stba.h)
    def set_inner_iterations(self, enable=True, tolerance=1e-3, rot_group=None, pos_group=None, pt_group=None):
        """a coordinate-descent sweep behind every valid step of solve() / lm_iterations().  rot_group, pos_group [n_cams] and
        pt_group [n_pts]: group id of every camera rotation, camera position and landmark (-1: not swept; equal rotation and
        position ids: one 6-dof camera block); all None: {cameras}, {landmarks}.  enable=False: off"""
        tol, r, q, p = inner_ordering(self.nc, self.np_, tolerance, rot_group, pos_group, pt_group)
        _chk(lib().stba_ba_set_inner_iterations(self._h, int(bool(enable)), C.c_double(tol), _p(r), _p(q), _p(p)),
             "stba_ba_set_inner_iterations")

    def inner_sweep(self):
        """one sweep at the current point, which moves the parameters: (cost before, cost after, inner LM iterations per block as
        a dict of int arrays rot [n_cams], pos [n_cams], pt [n_pts])"""
        c0, c1 = C.c_double(), C.c_double()
        it = np.zeros(2 * self.nc + self.np_, dtype=np.int32)
        _chk(lib().stba_ba_inner_sweep(self._h, C.byref(c0), C.byref(c1), _p(it)), "stba_ba_inner_sweep")
        return c0.value, c1.value, {"rot": it[: self.nc].copy(), "pos": it[self.nc: 2 * self.nc].copy(), "pt": it[2 * self.nc:].copy()}

    def inner_summary(self):
        """sweeps, the iteration that switched inner iterations off (-1: none), sweep device time (phase_timing) and group sizes
        of the last solve or sweep"""
        s = InnerSummary()
        s.struct_size = C.sizeof(InnerSummary)
        _chk(lib().stba_ba_last_inner_summary(self._h, C.byref(s)), "stba_ba_last_inner_summary")
        return s

    def time_schur_apply(self, reps=20):
        """ms per implicit product S x on the device (hipEvents), with the blocks and x of the last schur_apply"""
        ms = C.c_double()
        _chk(lib().stba_ba_time_schur_apply(self._h, int(reps), C.byref(ms)), "stba_ba_time_schur_apply")
        return ms.value

    def schur_apply(self, dc, dp, which=0, x=None):
        """S x (which 0), a preconditioner inverse applied to x (1 jacobi, 2 schur_jacobi), or the reduced rhs (x None), for the
        explicit diagonals dc [6 n_cams], dp [n_pts, 3]; needs normal_blocks() first"""
        y = np.zeros(6 * self.nc)
        _chk(lib().stba_ba_schur_apply(self._h, _p(_f64(dc)), _p(_f64(dp)), int(which), _p(None if x is None else _f64(x)), _p(y)),
             "stba_ba_schur_apply")
        return y

    def time_schur(self, reps=10):
        """(ms per launch of the Schur-complement kernel, LDS atomics per launch, observation pairs per launch)"""
        ms, at, pr = C.c_double(), C.c_double(), C.c_double()
        _chk(lib().stba_ba_time_schur(self._h, int(reps), C.byref(ms), C.byref(at), C.byref(pr)), "stba_ba_time_schur")
        return ms.value, at.value, pr.value


class PCGOptions(C.Structure):
    _fields_ = [("max_iterations", C.c_int), ("relative_tolerance", C.c_double), ("check_every", C.c_int),
                ("forcing_eta0", C.c_double), ("forcing_eta_min", C.c_double), ("coarse_group", C.c_int),
                ("coarse_refresh_every", C.c_int), ("one_kernel_solve", C.c_int),
                ("coarse_async", C.c_int), ("forcing_eta_final", C.c_double), ("coarse_eta", C.c_double), ("coarse_async_after", C.c_int),
                ("coarse_async_decrease", C.c_double)]


class PCGSummary(C.Structure):
    _fields_ = [("iterations_total", C.c_int), ("solves", C.c_int), ("hit_cap", C.c_int), ("max_iterations_in_a_solve", C.c_int),
                ("coarse_dim", C.c_int), ("coarse_refreshes", C.c_int), ("last_eta", C.c_double),
                ("coarse_failures", C.c_int), ("one_kernel_solves", C.c_int), ("linear_solve_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class PGCovarianceOptions(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("relative_tolerance", C.c_double), ("max_iterations", C.c_int), ("check_every", C.c_int)]


class PGCovarianceSummary(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("batches", C.c_int), ("columns", C.c_int), ("iterations_total", C.c_int),
                ("max_iterations_in_a_batch", C.c_int), ("max_relative_residual", C.c_double), ("device_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "struct_size"}


def pg_covariance_options(**kw):
    o = PGCovarianceOptions()
    lib().stba_pg_covariance_default_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def pg_gauge_check(n_nodes, edge_i, edge_j, node_fixed=None):
    """raises StbaError(STBA_ERR_NOT_POSITIVE_DEFINITE) if a connected component of the graph holds no constant node; host only"""
    ei = np.ascontiguousarray(edge_i, dtype=np.int32); ej = np.ascontiguousarray(edge_j, dtype=np.int32)
    nf = None if node_fixed is None else np.ascontiguousarray(node_fixed, dtype=np.uint8)
    _chk(lib().stba_pg_gauge_check(int(n_nodes), len(ei), _p(ei), _p(ej), _p(nf)), "stba_pg_gauge_check")


# robust loss kinds of the pose graph: the STBA_LOSS_* of include/stba.h by name (None and "trivial": no loss on that edge)
LOSS_KINDS = {None: 0, "trivial": 0, "huber": 1, "softlone": 2, "cauchy": 3, "arctan": 4, "tolerant": 5, "tukey": 6}


def pg_loss_table(m, kind, a=None, b=None, scale=None, who="PGEngine", what="edge"):
    """the per-edge table stba_pg_set_loss takes, from one spec for all m edges or per-edge sequences: kind a name of LOSS_KINDS (or
    its integer), a / b / scale numbers; each may be a scalar or have length m.  Returns (kind int32[m], a, b, scale float64[m]);
    a and b default to 1 where the kind does not use them, scale to 1.  Raises ValueError on an unknown name or a wrong length."""
    def code(k):
        if isinstance(k, (int, np.integer)) and not isinstance(k, bool):
            return int(k)
        key = k.lower() if isinstance(k, str) else k
        if key not in LOSS_KINDS:
            raise ValueError(f"{who}: unknown loss kind {k!r} (one of {sorted(x for x in LOSS_KINDS if x)} or None)")
        return LOSS_KINDS[key]

    if kind is None or isinstance(kind, (str, int, np.integer)):
        kinds = np.full(m, code(kind), np.int32)
    else:
        kinds = np.array([code(k) for k in kind], np.int32)
        if kinds.shape != (m,):
            raise ValueError(f"{who}: per-{what} loss kinds must have length {m}, got {kinds.shape}")

    def column(v, name):
        if v is None:
            return np.ones(m)
        v = np.asarray(v, np.float64)
        if v.ndim == 0:
            return np.full(m, float(v))
        if v.shape != (m,):
            raise ValueError(f"{who}: per-{what} loss parameter {name} must be a number or have length {m}, got {v.shape}")
        return np.ascontiguousarray(v)

    return kinds, column(a, "a"), column(b, "b"), column(scale, "scale")


class PGEngine:
    """Device-resident pose graph (BASELINE config C4, build-defined)."""

    def __init__(self, poses, edge_i, edge_j, meas, node_fixed=None, stream=None, information=None, sqrt_information=None, loss=None,
                 priors=None):
        """information / sqrt_information: (m, 6, 6) per-edge weights (set_information / set_sqrt_information); at most one of them.
        loss: a kind name ("huber" uses a = 1), a tuple (kind, a[, b[, scale]]) or a dict of set_loss's arguments.
        priors: a dict of set_priors' arguments (nodes=, poses=, information= | sqrt_information=)"""
        self._h = C.c_void_p()
        if information is not None and sqrt_information is not None:
            raise ValueError("PGEngine: give information or sqrt_information, not both")
        poses = _f64(poses).reshape(-1, 7)
        ei = np.ascontiguousarray(edge_i, dtype=np.int32); ej = np.ascontiguousarray(edge_j, dtype=np.int32)
        meas = _f64(meas).reshape(-1, 7)
        nf = None if node_fixed is None else np.ascontiguousarray(node_fixed, dtype=np.uint8)
        self.n, self.m = len(poses), len(ei)
        weights = None if information is None and sqrt_information is None else \
            self._edge_blocks(information if information is not None else sqrt_information)
        table = None if loss is None else self._loss_table(loss)
        _chk(lib().stba_pg_create(C.byref(self._h), self.n, self.m, _p(poses), _p(ei), _p(ej), _p(meas), _p(nf),
                                  C.c_void_p(stream or 0)), "stba_pg_create")
        if table is not None:
            self._set_loss_table(table)
        if information is not None:
            self.set_information(weights)
        elif sqrt_information is not None:
            self.set_sqrt_information(weights)
        if priors is not None:
            try:
                self.set_priors(**priors)
            except Exception:
                self.close()
                raise

    # ---- node pose priors
    def set_priors(self, nodes, poses=None, information=None, sqrt_information=None):
        """soft constraints on node poses (stba_pg_set_priors): prior k pulls node nodes[k] towards poses[k] = [qx, qy, qz, qw, tx, ty,
        tz] with cost 1/2 |W_k r_k|^2, r_k = log(Z_k^-1 T) in the tangent order [rho(3), theta(3)].  information: (n, 6, 6) symmetric
        positive definite (W = L^T of its Cholesky factor) or sqrt_information: (n, 6, 6) any finite W (zero theta rows: a
        position-only prior); a single (6, 6) is taken for every prior, an (n,) array of sigmas means I / sigma; neither: the
        identity.  Several priors may name one node.  nodes empty (or None) clears the priors."""
        if information is not None and sqrt_information is not None:
            raise ValueError("PGEngine: give information or sqrt_information, not both")
        c = np.ascontiguousarray([] if nodes is None else nodes, dtype=np.int32).reshape(-1)
        n = len(c)
        if n == 0:
            _chk(lib().stba_pg_set_priors(self._h, 0, None, None, None, None), "stba_pg_set_priors")
            return
        ps = _f64(poses).reshape(-1, 7)
        if len(ps) != n:
            raise ValueError(f"PGEngine: {n} prior nodes but {len(ps)} prior poses")

        def blocks(w, name, power):
            if w is None:
                return None
            w = np.asarray(w, np.float64)
            if w.shape == (n,):                           # sigmas: W = I / sigma, Omega = I / sigma^2
                w = np.eye(6)[None, :, :] / (w ** power)[:, None, None]
            if w.shape == (6, 6):
                w = np.broadcast_to(w, (n, 6, 6))
            if w.shape != (n, 6, 6):
                raise ValueError(f"PGEngine: prior {name} must have shape (6, 6), ({n}, 6, 6) or ({n},), got {w.shape}")
            return np.ascontiguousarray(w)
        om, w = blocks(information, "information", 2), blocks(sqrt_information, "sqrt_information", 1)
        _chk(lib().stba_pg_set_priors(self._h, n, _p(c), _p(ps), _p(om), _p(w)), "stba_pg_set_priors")

    def prior_count(self):
        n = C.c_int()
        _chk(lib().stba_pg_prior_count(self._h, C.byref(n)), "stba_pg_prior_count")
        return n.value

    def evaluate_priors(self, jac=True):
        """(cost, r [n, 6], J [n, 6, 6] | None) of the priors alone at the current poses: whitened, in the order they were set"""
        n = self.prior_count()
        cost = C.c_double()
        r = np.zeros((n, 6))
        J = np.zeros((n, 6, 6)) if jac else None
        _chk(lib().stba_pg_evaluate_priors(self._h, C.byref(cost), _p(r), _p(J)), "stba_pg_evaluate_priors")
        return cost.value, r, J

    def prior_kernel_geometry(self):
        """(priors per workgroup of the per-prior kernel, prior-bearing nodes per workgroup of the per-node kernel): a diagnostic"""
        a, b = C.c_int(), C.c_int()
        _chk(lib().stba_pg_prior_kernel_geometry(self._h, C.byref(a), C.byref(b)), "stba_pg_prior_kernel_geometry")
        return a.value, b.value

    def _edge_blocks(self, a):
        a = _f64(a)
        if a.size != self.m * 36 or a.shape[0] != self.m:
            raise ValueError(f"PGEngine: per-edge weights must have shape ({self.m}, 6, 6), got {a.shape}")
        return a.reshape(self.m, 36)

    def set_information(self, information):
        """per-edge information matrices Omega (m, 6, 6), symmetric positive definite, tangent order [rho, theta]: the cost becomes
        1/2 sum r^T Omega r.  Factored on the device as Omega = L L^T, W = L^T (include/stba.h).  None: back to the identity."""
        a = None if information is None else self._edge_blocks(information)
        _chk(lib().stba_pg_set_information(self._h, _p(a)), "stba_pg_set_information")

    def set_sqrt_information(self, sqrt_information):
        """per-edge square-root information W (m, 6, 6), any finite matrices: the cost becomes 1/2 sum |W r|^2.  None: identity."""
        a = None if sqrt_information is None else self._edge_blocks(sqrt_information)
        _chk(lib().stba_pg_set_sqrt_information(self._h, _p(a)), "stba_pg_set_sqrt_information")

    @property
    def has_information(self):
        has = C.c_int()
        _chk(lib().stba_pg_has_information(self._h, C.byref(has)), "stba_pg_has_information")
        return bool(has.value)

    def _loss_table(self, loss):
        if isinstance(loss, dict):
            return pg_loss_table(self.m, **loss)
        if isinstance(loss, tuple):
            return pg_loss_table(self.m, *loss)
        return pg_loss_table(self.m, loss)

    def _set_loss_table(self, table):
        kind, a, b, scale = table
        _chk(lib().stba_pg_set_loss(self._h, _p(kind), _p(a), _p(b), _p(scale)), "stba_pg_set_loss")

    def set_loss(self, kind, a=None, b=None, scale=None):
        """robust losses (Ceres' kinds, LOSS_KINDS): the cost becomes 1/2 sum rho_e(|W_e r_e|^2).  One spec for all edges --
        set_loss("cauchy", 0.5) -- or per-edge sequences of length m: set_loss(["huber", None, ...], a_array).  b is TolerantLoss'
        second parameter; scale multiplies the loss (ScaledLoss).  evaluate() then returns the corrected r and J, covariance()
        (J'^T J')^-1 (include/stba.h).  set_loss(None): no loss, the engine as it was."""
        if kind is None and a is None and b is None and scale is None:
            _chk(lib().stba_pg_set_loss(self._h, None, None, None, None), "stba_pg_set_loss")
            return
        self._set_loss_table(pg_loss_table(self.m, kind, a, b, scale))

    @property
    def has_loss(self):
        has = C.c_int()
        _chk(lib().stba_pg_has_loss(self._h, C.byref(has)), "stba_pg_has_loss")
        return bool(has.value)

    def close(self):
        if self._h:
            lib().stba_pg_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_allreduce(self, fn, rank, world):
        cb = ALLREDUCE_FN(fn)
        self._keep = getattr(self, "_keep", []) + [cb]
        _chk(lib().stba_pg_set_allreduce(self._h, cb, None, rank, world), "stba_pg_set_allreduce")

    def set_comm(self, comm):
        """edge shard of a multi-GPU solve: cross-rank sums through a native RCCL communicator"""
        self._keep = getattr(self, "_keep", []) + [comm]
        _chk(lib().stba_pg_set_comm(self._h, comm._h if comm is not None else None), "stba_pg_set_comm")

    def get_poses(self):
        out = np.zeros((self.n, 7))
        _chk(lib().stba_pg_get_poses(self._h, _p(out)), "stba_pg_get_poses")
        return out

    def evaluate(self, jac=True):
        cost = C.c_double()
        r = np.zeros((self.m, 6))
        Ji = np.zeros((self.m, 6, 6)) if jac else None
        Jj = np.zeros((self.m, 6, 6)) if jac else None
        _chk(lib().stba_pg_evaluate(self._h, C.byref(cost), _p(r), _p(Ji), _p(Jj)), "stba_pg_evaluate")
        return cost.value, r, Ji, Jj

    def time_kernels(self, reps=50):
        """(ms per residual+Jacobian launch, ms per matrix-free product), hipEvent-timed on the device"""
        a, b = C.c_double(), C.c_double()
        _chk(lib().stba_pg_time_kernels(self._h, int(reps), C.byref(a), C.byref(b)), "stba_pg_time_kernels")
        return a.value, b.value

    def pcg_options(self, **kw):
        pcg = PCGOptions()
        lib().stba_pcg_default_options(C.byref(pcg))
        for k, v in kw.items():
            setattr(pcg, k, v)
        return pcg

    def pcg_summary(self):
        """linear-solver side of the last solve(): PCG iterations, solves that hit the cap, coarse dimension, ..."""
        out = PCGSummary()
        _chk(lib().stba_pg_last_pcg_summary(self._h, C.byref(out)), "stba_pg_last_pcg_summary")
        return out

    def solve(self, opt=None, pcg=None, **kw):
        opt = opt or default_options(**kw)
        if pcg is None:
            pcg = self.pcg_options()
        trace = np.zeros((opt.max_num_iterations + 1, TRACE_COLS))
        summ = LMSummary()
        total = C.c_int()
        _chk(lib().stba_pg_solve(self._h, C.byref(opt), C.byref(pcg), C.byref(summ), _p(trace), C.byref(total)),
             "stba_pg_solve")
        return summ, trace[: summ.num_iterations + 1], total.value

    def covariance(self, pairs, **opt):
        """(n_pairs, 6, 6): the blocks C[a, b] of (J^T J)^-1 at the current poses, tangent [rho, theta]; and the summary as a dict.
        opt: relative_tolerance, max_iterations, check_every (stba_pg_covariance_options)"""
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        a = np.ascontiguousarray(pairs[:, 0]); b = np.ascontiguousarray(pairs[:, 1])
        out = np.zeros((len(pairs), 6, 6))
        summ = PGCovarianceSummary(struct_size=C.sizeof(PGCovarianceSummary))
        o = pg_covariance_options(**opt)
        _chk(lib().stba_pg_covariance(self._h, len(pairs), _p(a), _p(b), C.byref(o), _p(out), C.byref(summ)), "stba_pg_covariance")
        return out, summ.as_dict()

    def covariance_columns(self, node, **opt):
        """(6 n, 6): the six columns of (J^T J)^-1 that belong to `node` -- its covariance with every pose; and the summary as a dict"""
        out = np.zeros((6 * self.n, 6))
        summ = PGCovarianceSummary(struct_size=C.sizeof(PGCovarianceSummary))
        o = pg_covariance_options(**opt)
        _chk(lib().stba_pg_covariance_columns(self._h, int(node), C.byref(o), _p(out), C.byref(summ)), "stba_pg_covariance_columns")
        return out, summ.as_dict()


def cholesky_factor(A, stream=None):
    A = _f64(A).copy()
    _chk(lib().stba_cholesky_factor(_p(A), A.shape[0], C.c_void_p(stream or 0)), "stba_cholesky_factor")
    return np.tril(A)


def cholesky_solve(A, b, stream=None):
    A = _f64(A); x = _f64(b).copy()
    _chk(lib().stba_cholesky_solve(_p(A), A.shape[0], _p(x), C.c_void_p(stream or 0)), "stba_cholesky_solve")
    return x


def cholesky_inverse(A, stream=None):
    """(A^-1, pivot ratio) by the routine behind the covariances (stba_cholesky_inverse): the partial factorisation of [A .; I 0]"""
    A = _f64(A)
    Ainv = np.zeros_like(A); rc = C.c_double()
    _chk(lib().stba_cholesky_inverse(_p(A), A.shape[0], _p(Ainv), C.byref(rc), C.c_void_p(stream or 0)), "stba_cholesky_inverse")
    return Ainv, rc.value


def cholesky_time(n, reps=5, stream=None):
    ms = C.c_double()
    _chk(lib().stba_cholesky_time(int(n), int(reps), C.byref(ms), C.c_void_p(stream or 0)), "stba_cholesky_time")
    return ms.value


def cholesky_schedule_model(n, n_xcd=8, wg_per_xcd=32):
    """Host-only: makespan (us) the scheduling model predicts for the persistent factorisation kernel."""
    out = C.c_double()
    _chk(lib().stba_cholesky_schedule_model(int(n), int(n_xcd), int(wg_per_xcd), C.byref(out)), "stba_cholesky_schedule_model")
    return out.value


def cholesky_set_timeout_us(us):
    """bound on a workgroup's wait for a dependency inside the persistent factorisation (0: automatic)"""
    _chk(lib().stba_cholesky_set_timeout_us(C.c_double(us)), "stba_cholesky_set_timeout_us")


def cholesky_timeout_count():
    """how often the persistent factorisation gave up (shared device) and the stage kernels took over, in this process"""
    return int(lib().stba_cholesky_timeout_count())


def cholesky_shard_model(n, n_gpus, n_xcd=8, wg_per_xcd=32, rows_per_group=0, hop_us=3.0, link_gb_per_s=48.0):
    """Host-only design study: (makespan us, cross-GPU dependencies, remote 128x128 tiles fetched by the busiest GPU)
    of the factorisation's task graph spread block-cyclically over n_gpus GPUs (include/stba.h)."""
    ms = C.c_double(); ce = C.c_double(); ti = C.c_double()
    _chk(lib().stba_cholesky_shard_model(int(n), int(n_gpus), int(n_xcd), int(wg_per_xcd), int(rows_per_group), C.c_double(hop_us),
                                         C.c_double(link_gb_per_s), C.byref(ms), C.byref(ce), C.byref(ti)), "stba_cholesky_shard_model")
    return ms.value, ce.value, ti.value


def cholesky_shard_owner(n_block_rows, n_gpus, rows_per_group):
    """tile row -> GPU of the block-cyclic distribution of the sharded-solve design"""
    out = np.zeros(int(n_block_rows), np.int32)
    _chk(lib().stba_cholesky_shard_owner(int(n_block_rows), int(n_gpus), int(rows_per_group), out.ctypes.data_as(C.POINTER(C.c_int))),
         "stba_cholesky_shard_owner")
    return out


def cholesky_time_split(n, reps=5, stream=None):
    """(ms_factor, ms_backward) of the production schedule, hipEvent-timed on the device"""
    a = C.c_double(); b = C.c_double()
    _chk(lib().stba_cholesky_time_split(int(n), int(reps), C.byref(a), C.byref(b), C.c_void_p(stream or 0)),
         "stba_cholesky_time_split")
    return a.value, b.value


def cholesky_profile(n, stream=None):
    ms = np.zeros(4); fl = C.c_double(); flp = C.c_double(); nl = C.c_int()
    _chk(lib().stba_cholesky_profile(int(n), _p(ms), C.byref(fl), C.byref(flp), C.byref(nl), C.c_void_p(stream or 0)),
         "stba_cholesky_profile")
    return dict(ms_diag=ms[0], ms_trsm=ms[1], ms_syrk=ms[2], ms_bwd=ms[3], syrk_flops=fl.value,
                syrk_flops_padded=flp.value, syrk_launches=nl.value)


def two_view_init(f1, f2, K, points=True, stream=None):
    """two_view_geometry.cpp:18-126 on the device: pixel pairs (n, 2) x 2 and K -> dict(F, R, t, pts, fails);
    (R, t) = pose of frame 2 in frame 1, |t| = 1.  Raises StbaError (no solution) like the reference's empty optional."""
    f1, f2, K = _f64(f1), _f64(f2), _f64(K)
    n = f1.shape[0]
    F = np.zeros((3, 3)); R = np.zeros((3, 3)); t = np.zeros(3)
    pts = np.zeros((n, 3)) if points else None
    fails = np.zeros(4, dtype=np.int32)
    _chk(lib().stba_two_view_init(n, _p(f1), _p(f2), _p(K), _p(F), _p(R), _p(t), _p(pts) if points else None,
                                  fails.ctypes.data_as(C.POINTER(C.c_int)), C.c_void_p(stream or 0)), "stba_two_view_init")
    return dict(F=F, R=R, t=t, pts=pts, fails=fails)


def odometry_read(path):
    """odometry file (st16 scene.cpp:66-110) -> (stamps[n], poses[n, 7] = qx qy qz qw x y z)"""
    n = C.c_int()
    _chk(lib().stba_odometry_read(path.encode(), C.byref(n), None, None, 0), "stba_odometry_read")
    stamps = np.zeros(n.value); poses = np.zeros((n.value, 7))
    _chk(lib().stba_odometry_read(path.encode(), C.byref(n), _p(stamps), _p(poses), n.value), "stba_odometry_read")
    return stamps, poses


def odometry_write(path, stamps, poses):
    poses = _f64(poses).reshape(-1, 7)
    st_ = None if stamps is None else _f64(stamps)
    _chk(lib().stba_odometry_write(path.encode(), len(poses), _p(st_), _p(poses)), "stba_odometry_write")


def trajectory_ate(truth, estimate):
    """absolute trajectory error (st4 pose_simulation.cpp:198-209) of two (n, 7) pose sequences"""
    a, b = _f64(truth).reshape(-1, 7), _f64(estimate).reshape(-1, 7)
    out = C.c_double()
    _chk(lib().stba_trajectory_ate(len(a), _p(a), _p(b), C.byref(out)), "stba_trajectory_ate")
    return out.value


def corners_read(path):
    """chessboard corner file -> (rows, cols, xy[rows, cols, 2])  (cbcorner.cpp:50-73)"""
    r = C.c_int(); c = C.c_int()
    _chk(lib().stba_corners_read(path.encode(), C.byref(r), C.byref(c), None, 0), "stba_corners_read")
    xy = np.zeros((r.value, c.value, 2))
    _chk(lib().stba_corners_read(path.encode(), C.byref(r), C.byref(c), _p(xy), r.value * c.value), "stba_corners_read")
    return r.value, c.value, xy


def corners_write(path, xy):
    xy = _f64(xy)
    _chk(lib().stba_corners_write(path.encode(), xy.shape[0], xy.shape[1], _p(xy)), "stba_corners_write")


def zhang_init(obj, img):
    """closed-form calibration start (calib.cpp:55-173): obj, img (V, C, 2) -> (params[9 + 6V], H[V, 3, 3])"""
    obj, img = _f64(obj), _f64(img)
    V, Cn = obj.shape[0], obj.shape[1]
    params = np.zeros(9 + 6 * V); H = np.zeros((V, 3, 3))
    _chk(lib().stba_zhang_init(V, Cn, _p(obj), _p(img), _p(params), _p(H)), "stba_zhang_init")
    return params, H


def calib_evaluate(params, obj, img, jac=True):
    """st3 calibration residual / Jacobian kernel.  obj, img: (V, C, 2)"""
    obj, img = _f64(obj), _f64(img)
    V, Cn = obj.shape[0], obj.shape[1]
    sse = C.c_double()
    e = np.zeros((V, Cn, 2))
    Ji = np.zeros((V, Cn, 2, 9)) if jac else None
    Jx = np.zeros((V, Cn, 2, 6)) if jac else None
    _chk(lib().stba_calib_evaluate(V, Cn, _p(_f64(params)), _p(obj), _p(img), C.byref(sse), _p(e), _p(Ji), _p(Jx)),
         "stba_calib_evaluate")
    return sse.value, e, Ji, Jx


def calib_gauss_newton(params, obj, img, max_iter=10):
    """CalibSolver::totalOptimization on the device; returns (params, iterations, sse_trace)"""
    params = _f64(params).copy()
    obj, img = _f64(obj), _f64(img)
    V, Cn = obj.shape[0], obj.shape[1]
    tr = np.full(max_iter, np.nan)
    it = C.c_int()
    _chk(lib().stba_calib_gauss_newton(V, Cn, _p(params), _p(obj), _p(img), int(max_iter), _p(tr), C.byref(it)),
         "stba_calib_gauss_newton")
    return params, it.value, tr


def _residual_callback(residual, n_params, n_res, n_local):
    def _fn(_u, xp, rp, Jp):
        xx = np.ctypeslib.as_array(xp, shape=(n_params,)).copy()
        r, J = residual(xx)
        np.ctypeslib.as_array(rp, shape=(n_res,))[:] = r
        if Jp:
            np.ctypeslib.as_array(Jp, shape=(n_res * n_local,))[:] = np.asarray(J, dtype=np.float64).reshape(-1)
        return 0
    return _fn


def dense_solve(residual, x0, n_res, n_local=None, plus=None, lower=None, upper=None, opt=None, callback=None, **kw):
    """residual(x) -> (r[n_res], J[n_res, n_local] or None-ignored); plus(x, d) -> x_new.
    The residual/Jacobian callback runs on the host (it is user code, like
    CostFunction::Evaluate); normal equations and the damped Cholesky step run on the device."""
    x = _f64(x0).copy()
    n_params = x.size
    n_local = n_local or n_params
    _fn = _residual_callback(residual, n_params, n_res, n_local)

    def _plus(_u, xp, dp, op):
        xx = np.ctypeslib.as_array(xp, shape=(n_params,)).copy()
        dd = np.ctypeslib.as_array(dp, shape=(n_local,)).copy()
        np.ctypeslib.as_array(op, shape=(n_params,))[:] = plus(xx, dd)

    opt = opt or default_options(**kw)
    trace = np.zeros((opt.max_num_iterations + 1, TRACE_COLS))
    summ = LMSummary()
    cfn = RESIDUAL_FN(_fn)
    cplus = PLUS_FN(_plus) if plus is not None else C.cast(None, PLUS_FN)
    cb = ITER_CB(callback) if callback else C.cast(None, ITER_CB)
    lo = None if lower is None else _f64(lower)
    up = None if upper is None else _f64(upper)
    _chk(lib().stba_dense_solve(cfn, cplus, None, n_params, n_local, n_res, _p(x), _p(lo), _p(up), C.byref(opt),
                                C.byref(summ), _p(trace), cb, None), "stba_dense_solve")
    return x, summ, trace[: summ.num_iterations + 1]


def dense_covariance(residual, x, n_res, n_local=None, min_rcond=1e-14):
    """(J^T J)^-1 at x (stba_dense_covariance): residual(x) -> (r[n_res], J[n_res, n_local]) as in dense_solve, evaluated once
    on the host; J^T J and its inverse on the device.  Returns (cov [n_local, n_local], rcond = the pivot ratio of J^T J)."""
    x = _f64(x)
    n_params = x.size
    n_local = n_local or n_params
    cfn = RESIDUAL_FN(_residual_callback(residual, n_params, n_res, n_local))
    cov = np.zeros((n_local, n_local))
    rc = C.c_double()
    _chk(lib().stba_dense_covariance(cfn, None, n_params, n_local, n_res, _p(x), C.c_double(min_rcond), _p(cov), C.byref(rc)),
         "stba_dense_covariance")
    return cov, rc.value
