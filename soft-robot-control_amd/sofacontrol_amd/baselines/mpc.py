"""Linear MPC on the LOCP QP with the trust region switched off (sofacontrol/baselines/ros.py:14-136:
`runMPCSolver`, `MPCSolver`; 139-235: `MPCSolverNode` in-process, with `MPCClient` and the resident `KoopmanSolverNode`).  Constant (A_d, B_d, d_d)
over the horizon, the same HIP QP kernel as GuSTO's LOCP (`is_tr_active=False`, locp.py:57)."""
import numpy as np
from scipy.interpolate import interp1d

from ..scp.locp import LOCP


def runMPCSolver(model, N, dt, cost_params, x0, target, U=None, X=None, Xf=None, dU=None, verbose=0, warm_start=True,
                 **kwargs):
    """baselines/ros.py:14-28 without the ROS spin: build the solver, return its first solution."""
    return MPCSolver(model, N, dt, cost_params, x0, target, U=U, X=X, Xf=Xf, dU=dU, verbose=verbose,
                     warm_start=warm_start, **kwargs).get_solution()


class MPCSolver:
    def __init__(self, model, horizon, dt, cost_params, x0, target, U=None, X=None, Xf=None, dU=None, verbose=0,
                 warm_start=True, **kwargs):
        self.model = model
        self.planning_horizon = horizon
        self.dt = dt
        self.target = target
        self.cost_params = cost_params
        if self.target.z is not None and self.target.z.ndim == 2:
            self.z_interp = interp1d(self.target.t, self.target.z, axis=0, bounds_error=False,
                                     fill_value=(self.target.z[0, :], self.target.z[-1, :]))
        if self.target.u is not None and self.target.u.ndim == 2:
            self.u_interp = interp1d(self.target.t, self.target.u, axis=0, bounds_error=False,
                                     fill_value=(self.target.u[0, :], self.target.u[-1, :]))
        self.verbose = verbose
        self.locp = LOCP(self.planning_horizon, self.model.H, self.cost_params.Q, self.cost_params.R,
                         Qzf=self.cost_params.Qf, U=U, X=X, Xf=Xf, dU=dU, verbose=(verbose == 2), warm_start=warm_start,
                         is_tr_active=False, **kwargs)
        self.A_d = [self.model.A_d for _ in range(self.planning_horizon)]
        self.B_d = [self.model.B_d for _ in range(self.planning_horizon)]
        if hasattr(self.model, 'd_d'):
            self.d_d = [self.model.d_d for _ in range(self.planning_horizon)]
        else:
            self.d_d = [np.zeros(self.model.A_d.shape[0]) for _ in range(self.planning_horizon)]
        self.X = X
        self.xopt = self.uopt = self.zopt = self.topt = None
        self.solve(0.0, np.asarray(x0, dtype=np.float64).ravel())

    def solve(self, t0, x0):
        """One receding-horizon solve (constructor body 79-99 and MPC_callback 159-184 of baselines/ros.py)."""
        z, zf, u = self.get_target(t0)
        self.locp.update(self.A_d, self.B_d, self.d_d, x0, None, 0, 0, z=z, zf=zf, u=u)
        Jstar, success, stats = self.locp.solve()
        if success:
            if self.verbose:
                print('{:.3f} s from LOCP solve'.format(stats.solve_time))
            self.xopt, self.uopt, _ = self.locp.get_solution()
            self.Jstar, self.solve_time = Jstar, stats.solve_time
        else:
            print('No solution found, extending previous solution')
            self.xopt = np.concatenate((self.xopt[1:, :], np.expand_dims(self.xopt[-1, :], axis=0)), axis=0)
            self.uopt = np.concatenate((self.uopt[1:, :], np.expand_dims(self.uopt[-1, :], axis=0)), axis=0)
        return success

    def get_solution(self):
        self.zopt = np.transpose(self.model.H @ self.xopt.T)
        self.topt = self.dt * np.arange(self.planning_horizon + 1)
        return self.xopt, self.uopt, self.zopt, self.topt

    def get_target(self, t0):
        """baselines/ros.py:101-135 (constant targets are tiled per step)."""
        N = self.planning_horizon
        t = t0 + self.dt * np.arange(N + 1)
        if self.target.z is not None:
            z = self.z_interp(t) if self.target.z.ndim == 2 else np.tile(self.target.z.reshape(1, -1), (N + 1, 1))
        else:
            z = None
        zf = z[-1, :] if (self.cost_params.Qf is not None and z is not None) else None
        if self.target.u is not None:
            u = self.u_interp(t)[:N] if self.target.u.ndim == 2 else np.tile(self.target.u.reshape(1, -1), (N, 1))
        else:
            u = None
        return z, zf, u


class MPCSolverNode:
    """In-process form of the reference's ROS service node (baselines/ros.py:139-235): the LOCP with is_tr_active=False and
    constant A_d, B_d is built once; `mpc_callback(t0, x0)` answers one request.  On a failed solve the previous solution is
    shifted by one step (ros.py:223-227)."""

    def __init__(self, model, horizon, dt, cost_params, target, U=None, X=None, Xf=None, dU=None, verbose=0, warm_start=True,
                 **kwargs):
        self.model = model
        self.planning_horizon = horizon
        self.dt = dt
        self.target = target
        self.cost_params = cost_params
        if self.target.z is not None and self.target.z.ndim == 2:
            self.z_interp = interp1d(self.target.t, self.target.z, axis=0, bounds_error=False,
                                     fill_value=(self.target.z[0, :], self.target.z[-1, :]))
        if self.target.u is not None and self.target.u.ndim == 2:
            self.u_interp = interp1d(self.target.t, self.target.u, axis=0, bounds_error=False,
                                     fill_value=(self.target.u[0, :], self.target.u[-1, :]))
        self.verbose = verbose
        self.locp = LOCP(self.planning_horizon, self.model.H, self.cost_params.Q, self.cost_params.R,
                         Qzf=self.cost_params.Qf, U=U, X=X, Xf=Xf, dU=dU, verbose=(verbose == 2), warm_start=warm_start,
                         is_tr_active=False, **kwargs)
        N = self.planning_horizon
        self.A_d = [self.model.A_d for _ in range(N)]
        self.B_d = [self.model.B_d for _ in range(N)]
        if hasattr(self.model, 'd_d'):
            self.d_d = [self.model.d_d for _ in range(N)]
        else:
            self.d_d = [np.zeros(self.model.A_d.shape[0]) for _ in range(N)]
        self.X = X
        self.xopt = self.uopt = self.topt = None

    get_target = MPCSolver.get_target

    def mpc_callback(self, t0, x0):
        """ros.py:202-235: returns (t, xopt, uopt, zopt, solve_time)."""
        x0 = np.asarray(x0, dtype=np.float64).ravel()
        z, zf, u = self.get_target(t0)
        self.locp.update(self.A_d, self.B_d, self.d_d, x0, None, 0, 0, z=z, zf=zf, u=u)
        Jstar, success, stats = self.locp.solve()
        if success:
            self.xopt, self.uopt, _ = self.locp.get_solution()
            solve_time = stats.solve_time
        else:
            print('No solution found, extending previous solution')
            self.xopt = np.concatenate((self.xopt[1:, :], np.expand_dims(self.xopt[-1, :], axis=0)), axis=0)
            self.uopt = np.concatenate((self.uopt[1:, :], np.expand_dims(self.uopt[-1, :], axis=0)), axis=0)
            solve_time = 0.0
        self.topt = t0 + self.dt * np.arange(self.planning_horizon + 1)
        zopt = np.transpose(self.model.H @ self.xopt.T)
        return self.topt, self.xopt, self.uopt, zopt, solve_time


class MPCClient:
    """The MPCClientNode protocol of the reference (`send_request / check_if_done / force_wait / force_spin /
    get_solution(n_x, n_u)`) around an in-process `MPCSolverNode`: a request is answered at once."""

    def __init__(self, solver_node):
        self.node = solver_node
        self.sol = None

    def send_request(self, t0, x0, wait=True):
        self.sol = self.node.mpc_callback(t0, x0)

    def force_spin(self):
        pass

    def check_if_done(self):
        return self.sol is not None

    def force_wait(self):
        pass

    def get_solution(self, n_x, n_u):
        """(t, uopt, xopt, t_solve), as MPCClientNode.get_solution."""
        t, x, u, _, ts = self.sol
        return np.asarray(t), np.asarray(u).reshape(-1, n_u), np.asarray(x).reshape(-1, n_x), ts


class KoopmanSolverNode(MPCSolverNode):
    """MPCSolverNode of a Koopman model on the resident device plan (csrc/koopman.hip, skoop_mpc_*): the measurement ring,
    the lift W psi(zeta) into the QP's x0 and the QP itself stay on the device; A_d / B_d are tiled over the horizon once.
    `push(y, u_prev)` records one raw sample per problem; `solve_ring(t0)` is one step (lift -> QP -> one copy back).
    `batch` independent problems (same model, own histories) go through one launch: push / step take (batch x ...) arrays.
    Every node owns its lift handle and so its measurement history (KoopmanData per KoopmanMPC, as in the reference).  Of the
    LOCP options, `x_char` is taken (the QP's state scaling, as LOCP); `dU`, `input_nullspace` and `nonlinear_observer` are
    refused; solver settings (OSQP / GUROBI arguments) have no meaning for the device QP and are ignored, as LOCP does."""
    resident = True

    def __init__(self, model, horizon, dt, cost_params, target, U=None, X=None, Xf=None, dU=None, verbose=0, warm_start=True,
                 batch=1, **kwargs):
        import ctypes as C
        from .. import _lib
        from ..scp.locp import make_problem
        from .koopman.koopman_utils import _bind
        if dU is not None:
            raise RuntimeError('KoopmanSolverNode: input-rate constraints (dU) are not supported by the resident plan')
        for k in ('input_nullspace', 'nonlinear_observer'):
            if kwargs.get(k) is not None and kwargs.get(k) is not False:
                raise RuntimeError('KoopmanSolverNode: %s is not supported by the resident plan (use MPCSolverNode)' % k)
        super().__init__(model, horizon, dt, cost_params, target, U=U, X=X, Xf=Xf, dU=None, verbose=verbose,
                         warm_start=warm_start, **kwargs)
        self.batch = int(batch)
        self.lift = model.new_lift(project=True, batch=self.batch)
        x_char = kwargs.get('x_char')
        x_scale = None if x_char is None else 1. / np.abs(np.asarray(x_char, dtype=np.float64))
        n = self.lift.n_out
        if model.A_d.shape != (n, n):
            raise RuntimeError('KoopmanSolverNode: A_d is %s but the lift writes %d states' % (model.A_d.shape, n))
        self._prob, self._keep = make_problem(horizon, np.asarray(model.H, dtype=np.float64), cost_params.Q, cost_params.R,
                                              cost_params.Qf, U, X, Xf, None, x_scale, tr_active=False)
        self._A = _lib.f64(model.A_d); self._B = _lib.f64(model.B_d)
        self._plan = C.c_void_p()
        _lib.check(_bind().skoop_mpc_create(C.byref(self._plan), self.lift._h, C.cast(C.byref(self._prob), C.c_void_p),
                                            _lib.dptr(self._A), _lib.dptr(self._B)), 'skoop_mpc_create')
        self._C = C
        self.n_x, self.n_u = n, model.B_d.shape[1]
        self.last_x0 = None
        self.last_status = None
        self.last_J = None

    def push(self, y, u_prev):
        self.lift.push(y, u_prev)

    def set_timing(self, on=True):
        """Bracket the parts of every following step with device events (skoop_mpc_set_timing)."""
        from .. import _lib
        from .koopman.koopman_utils import _bind
        _lib.check(_bind().skoop_mpc_set_timing(self._plan, 1 if on else 0), 'skoop_mpc_set_timing')

    def stats(self):
        """{'steps', 'waits_last_step': blocking host waits of the last step, and with timing on the last step's device ms:
        'pre_qp_ms' (push, targets, lift), 'qp_ms', 'copy_back_ms', 'device_ms'} (skoop_mpc_stats)."""
        import ctypes as C
        from .. import _lib
        from .koopman.koopman_utils import _bind
        n, w, ms = C.c_int64(), C.c_int64(), np.empty(4)
        _lib.check(_bind().skoop_mpc_stats(self._plan, C.byref(n), C.byref(w), _lib.dptr(ms)), 'skoop_mpc_stats')
        return dict(steps=n.value, waits_last_step=w.value, pre_qp_ms=ms[0], qp_ms=ms[1], copy_back_ms=ms[2], device_ms=ms[3])

    def _targets(self, t0):
        from .. import _lib
        z, zf, u = self.get_target(t0)
        rep = lambda a: None if a is None else _lib.f64(np.broadcast_to(np.ravel(a), (self.batch, np.size(a))))
        zf = None if self.cost_params.Qf is None else zf
        return rep(z), rep(zf), rep(u)

    def step(self, t0, y=None, u_prev=None):
        """One resident step for every problem: [push] -> lift -> QP -> copy back.  Returns x0 (batch x n_x),
        x (batch x N+1 x n_x), u (batch x N x n_u), J (batch), status (batch; 0 = solved)."""
        from .. import _lib
        from .koopman.koopman_utils import _bind
        B, N, n, m = self.batch, self.planning_horizon, self.n_x, self.n_u
        z, zf, ud = self._targets(t0)
        if y is not None:
            y = _lib.f64(np.reshape(y, (B, -1))); u_prev = _lib.f64(np.reshape(u_prev, (B, -1)))
        x0 = np.empty((B, n)); x = np.empty((B, N + 1, n)); u = np.empty((B, N, m)); J = np.empty(B)
        st = np.empty(B, dtype=np.int32)
        _lib.check(_bind().skoop_mpc_step(self._plan, _lib.dptr(y), _lib.dptr(u_prev), _lib.dptr(z), _lib.dptr(zf), _lib.dptr(ud),
                                          _lib.dptr(x0), _lib.dptr(x), _lib.dptr(u), _lib.dptr(J), _lib.iptr(st)), 'skoop_mpc_step')
        return x0, x, u, J, st

    def solve_ring(self, t0):
        """mpc_callback on the device ring of problem 0: (t, uopt, xopt, solve_time, x0) -- the failure shift of ros.py:223-227."""
        import time
        t_start = time.time()
        x0, x, u, J, st = self.step(t0)
        solve_time = time.time() - t_start
        self.last_x0, self.last_status, self.last_J = x0, st, J
        if st[0] == 0:
            self.xopt, self.uopt = x[0], u[0]
        else:
            print('No solution found, extending previous solution')
            self.xopt = np.concatenate((self.xopt[1:, :], np.expand_dims(self.xopt[-1, :], axis=0)), axis=0)
            self.uopt = np.concatenate((self.uopt[1:, :], np.expand_dims(self.uopt[-1, :], axis=0)), axis=0)
        self.topt = t0 + self.dt * np.arange(self.planning_horizon + 1)
        return self.topt, self.uopt, self.xopt, solve_time, x0[0]

    def __del__(self):
        try:
            if getattr(self, '_plan', None):
                from .koopman.koopman_utils import _bind
                _bind().skoop_mpc_destroy(self._plan)
                self._plan = None
        except Exception:
            pass
