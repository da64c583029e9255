"""Koopman MPC controller -- surface of sofacontrol/baselines/koopman/koopman.py:11-197.

The reference sends `W lift(zeta)` to a ROS MPC node every Ts (compute_policy, 75-125).  Here the solver side is in-process:
`client=` takes any object with the MPCClientNode protocol (baselines/ros.py; e.g. `baselines.mpc.MPCClient` around an
`MPCSolverNode`), and `solver_node=` a `baselines.mpc.KoopmanSolverNode`, whose resident plan keeps the measurement ring,
the lift and the QP on the device: the controller then pushes every sample to the device ring and a solve is one
`skoop_mpc_step` (no lift on the host)."""
import numpy as np
from scipy.interpolate import interp1d

from ...closed_loop_controller import TemplateController
from .koopman_utils import KoopmanData


class KoopmanMPC(TemplateController):
    """koopman.py:11-186.  The plan tape is the reference's own (interp1d over the stitched t_opt / u_opt, 'previous' when
    input_hold): tpwl/controllers.py's _PlanTape samples a plan on its grid and has no 'previous' hold, so it is not reused;
    the solve schedule (t_compute, recompute every rollout_horizon steps) is kept inline for the same reason -- it counts
    in Ts from the end of the delay, as evaluate (138-170) does."""

    def __init__(self, dyn_sys, delay=2, u0=None, wait=True, client=None, solver_node=None, **kwargs):
        super().__init__()
        self.dyn_sys = dyn_sys
        self.input_dim = self.dyn_sys.m
        self.state_dim = self.dyn_sys.N
        self.dt = self.dyn_sys.Ts
        self.observer = KoopmanObserver()
        self.Y = kwargs.get('Y')
        self.u0 = u0 if u0 is not None else np.zeros(self.input_dim)
        self.t_compute = 0.
        self.u = self.u0
        self.solve_times = []
        self.data = KoopmanData(self.dyn_sys.scale, self.dyn_sys.delays)
        self.rollout_horizon = kwargs.get('rollout_horizon', 1)
        self.input_hold = kwargs.get('input_hold', False)
        self.t_opt = None
        self.u_opt = None
        self.x_opt = None
        self.u_bar = None
        self.x_bar = None
        self.x_opt_full = None
        self.wait = wait
        self.t_next_solve = 0
        self.initiailzed = False
        self.resident = solver_node is not None and getattr(solver_node, 'resident', False)
        if client is None and solver_node is None:
            raise RuntimeError('KoopmanMPC needs client= (MPCClientNode protocol) or solver_node= (MPCSolverNode / KoopmanSolverNode)')
        if client is None and not self.resident:
            from ..mpc import MPCClient
            client = MPCClient(solver_node)
        self.node = solver_node
        self.MPC = client
        self.requests = []          # (t0, lifted x0) of every solve, for records and tests
        self.z_opt_horizon = []
        self.t_opt_horizon = []
        self.t_delay = delay

    def set_sim_timestep(self, dt):
        self.sim_dt = dt

    def compute_policy(self, t_step, zeta_belief):
        t0 = round(t_step, 4)
        if self.resident:
            # the device ring already holds the delay-embedded measurement: lift -> QP -> results in one step
            t_opt_p, u_opt_p, x_opt_p, t_solve, x0 = self.node.solve_ring(t0)
        else:
            # Projects to "dominant" Koopman modes if 'W' is defined. Else 'W' is identity
            x0 = np.dot(self.dyn_sys.W, np.asarray(self.dyn_sys.lift_data(*zeta_belief)))
            self.MPC.send_request(t0, x0, wait=True)
            if not self.MPC.check_if_done():
                print('GuSTO cannot provide real-time compatibility, consider modifying problem')
                self.MPC.force_wait()
            t_opt_p, u_opt_p, x_opt_p, t_solve = self.MPC.get_solution(self.state_dim, self.input_dim)
        self.requests.append((t0, np.array(x0, dtype=np.float64)))
        t_opt_p = np.round(t_opt_p, 4)
        u_opt_p = self.data.scaling.scale_up(u=u_opt_p)
        self.solve_times.append(t_solve)

        u_opt_intp = interp1d(t_opt_p, np.vstack((u_opt_p, u_opt_p[-1, :])), axis=0)
        x_opt_intp = interp1d(t_opt_p, x_opt_p, axis=0)
        if self.t_opt is None:
            t_opt_new = self.dt * np.arange(self.rollout_horizon + 1)
            self.t_opt = t_opt_new
            self.u_opt = u_opt_intp(t_opt_new)
            self.x_opt = x_opt_intp(t_opt_new)
            self.x_opt_full = np.expand_dims(x_opt_p, axis=0)
        else:
            t_opt_new = self.t_opt[-1] + self.dt * np.arange(self.rollout_horizon + 1)
            u_opt_new = u_opt_intp(t_opt_new)
            x_opt_new = x_opt_intp(t_opt_new)
            self.t_opt = np.round(np.concatenate((self.t_opt, t_opt_new[1:])), 4)
            self.u_opt = np.concatenate((self.u_opt[:-1, :], u_opt_new))
            self.x_opt = np.concatenate((self.x_opt, x_opt_new[1:, :]))
            self.x_opt_full = np.concatenate((self.x_opt_full, np.expand_dims(x_opt_p, axis=0)))

        self.z_opt_horizon.append(self.data.scaling.scale_up(y=(self.dyn_sys.H @ x_opt_p.T).T))
        self.t_opt_horizon.append(t_opt_p)
        kind = 'previous' if self.input_hold else 'linear'
        self.u_bar = interp1d(self.t_opt, self.u_opt, kind=kind, axis=0)
        self.x_bar = interp1d(self.t_opt, self.x_opt, kind=kind, axis=0)

    def recompute_policy(self, t_step):
        step = round(round(t_step, 4) / self.dt)
        return int(step % self.rollout_horizon) == 0

    def compute_input(self, t_step, z_belief):
        if not self.resident:
            self.MPC.force_spin()
        return self.u_bar(t_step)

    def evaluate(self, sim_time, y, x, u_prev):
        """koopman.py:138-170: the measurement is recorded at every simulation step; a solve every Ts * rollout_horizon."""
        sim_time = round(sim_time, 4)
        self.observer.update(None, y, None)
        if self.Y is not None and not self.Y.contains(y):
            y = self.Y.project_to_polyhedron(y)
        if self.resident:
            self.node.push(y, u_prev)
        else:
            self.data.add_measurement(y, u_prev)
        if round(sim_time, 4) < round(self.t_delay, 4):
            self.u = self.u0
        else:
            if round(sim_time - self.t_delay, 4) >= round(self.t_compute, 4):
                zeta_belief = None if self.resident else self.data.get_zeta()
                if self.recompute_policy(self.t_compute):
                    self.compute_policy(self.t_compute, zeta_belief)
                self.u = self.compute_input(self.t_compute, zeta_belief)
                self.t_compute = round(self.t_compute + self.dt, 4)
        self.u = np.atleast_1d(self.u)
        return self.u.copy()

    def save_controller_info(self):
        """koopman.py:172-186."""
        info = dict()
        info['t_opt'] = self.t_opt
        info['u_opt'] = self.u_opt
        info['z_opt'] = self.data.scaling.scale_up(y=(self.dyn_sys.H @ self.x_opt.T).T)
        info['zopt_full'] = self.data.scaling.scale_up(
            y=np.einsum("ij, klj -> ikl", self.dyn_sys.H, self.x_opt_full).T).transpose((1, 0, 2))
        info['z_rollout'] = self.z_opt_horizon
        info['t_rollout'] = self.t_opt_horizon
        info['solve_times'] = self.solve_times
        info['rollout_time'] = self.rollout_horizon * self.dt
        return info


class KoopmanObserver:
    """koopman.py:189-197."""

    def __init__(self):
        self.z = None

    def update(self, u, y, dt, x=None):
        self.z = y
