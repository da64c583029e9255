"""ROMPC controller -- surface of sofacontrol/baselines/rompc/rompc.py:10-150.

The reduced-order OCP is solved by an MPC node behind the MPCClientNode protocol (`client=`), or in-process by a
`baselines.mpc.MPCSolverNode` (`solver_node=`, wrapped in `baselines.mpc.MPCClient`).  Everything between two solves
runs on the device: an active step (feedback on the estimate + observer update) is one `srompc_step`, a start-up step
(re-initialisation from the full state + observer update with u0) is one `srompc_step` with the full state and the input."""
import numpy as np
from scipy.interpolate import interp1d

from ...closed_loop_controller import TemplateController
from ...lqr.lqr import dare
from .observer import DiscreteLuenbergerObserver


class ROMPC(TemplateController):
    def __init__(self, dyn_sys, cost, costL, dt, N_replan=None, delay=2, u0=None, wait=True, client=None, solver_node=None):
        super().__init__()
        if client is None and solver_node is None:
            raise RuntimeError('ROMPC needs client= (MPCClientNode protocol) or solver_node= (baselines.mpc.MPCSolverNode)')
        if client is None:
            from ..mpc import MPCClient
            client = MPCClient(solver_node)
        self.MPC = client
        self.node = solver_node
        self.dyn_sys = dyn_sys
        self.dt = dt
        self.input_dim = dyn_sys.get_input_dim()
        self.state_dim = dyn_sys.get_state_dim()
        self.t_compute = 0.
        self.t_delay = delay
        self.u0 = np.zeros(self.input_dim) if u0 is None else u0
        self.u = self.u0
        self.N_replan = 1 if N_replan is None else N_replan
        self.t_opt = self.u_opt = self.x_opt = None
        self.ubar = self.xbar = None
        self.solve_times = []
        self.requests = []            # (t0, x0) of every request sent, for records and tests
        self.wait = wait
        self.t_next_solve = 0
        self.initialized = False
        self.observer = DiscreteLuenbergerObserver(dyn_sys, costL.Q, costL.R)
        self.K, _ = dare(dyn_sys.A_d, dyn_sys.B_d, cost.Q, cost.R)

    # the feedback gain sits next to the observer gain in the device handle
    @property
    def K(self):
        return self.observer.K

    @K.setter
    def K(self, value):
        self.observer.K = value

    def _request(self, t0, x0, wait):
        self.requests.append((float(t0), np.array(x0, dtype=np.float64)))
        self.MPC.send_request(t0, x0, wait=wait)

    def evaluate(self, sim_time, y, x, u_prev):
        """rompc.py:57-89.  Until the first solve the estimate is re-initialised from the full state x on every call."""
        xf = None if self.initialized else x
        active = False
        if round(sim_time, 4) >= round(self.t_delay, 4) and round(sim_time - self.t_delay, 4) >= round(self.t_compute, 4):
            if round(self.t_compute, 4) >= round(self.t_next_solve, 4):
                if xf is not None:
                    # the first request carries the freshly initialised estimate, so that one has to come back first
                    self.observer.initialize(xf)
                    xf = None
                self.ubar, self.xbar = self.solve_OCP()
                print('t_sim = {:.3f}'.format(self.t_compute))
            active = True
        if active:
            self.u = self.observer.step(y, ubar=self.ubar(self.t_compute), xbar=self.xbar(self.t_compute), xf=xf)
            self.t_compute += self.dt
            self.MPC.force_spin()
        else:
            held = self.u0 if round(sim_time, 4) < round(self.t_delay, 4) else self.u
            self.u = self.observer.step(y, u=np.atleast_1d(held), xf=xf)
        self.u = np.atleast_1d(self.u)
        return self.u.copy()

    def solve_OCP(self):
        """rompc.py:91-107: collect the plan that is due (the very first one is requested here, from the estimate), then
        start the next solve from where the stitched plan ends."""
        first = not self.initialized
        if first:
            self._request(self.t_compute, self.observer.x, True)
            self.initialized = True
        plan = self.get_OCP_solution(init=first)
        self._request(self.t_opt[-1], self.x_opt[-1, :], self.wait)
        self.t_next_solve = round(self.t_opt[-1], 6)
        return plan

    def get_OCP_solution(self, init=False):
        """rompc.py:109-141: the first N_replan controller steps of the new plan are appended to the nominal trajectory;
        the plan's last input row is repeated so that the inputs interpolate over the whole horizon."""
        if not self.MPC.check_if_done():
            print('MPC cannot provide real-time compatibility, consider modifying problem')
            self.MPC.force_wait()
        t_p, u_p, x_p, t_solve = self.MPC.get_solution(self.state_dim, self.input_dim)
        self.solve_times.append(t_solve)
        u_of_t = interp1d(t_p, np.vstack((u_p, u_p[-1, :])), axis=0)
        x_of_t = interp1d(t_p, x_p, axis=0)
        grid = self.dt * np.arange(self.N_replan + 1)
        if init:
            self.t_opt, self.u_opt, self.x_opt = grid, u_of_t(grid), x_of_t(grid)
        else:
            grid = self.t_opt[-1] + grid
            self.t_opt = np.concatenate((self.t_opt, grid[1:]))
            self.u_opt = np.concatenate((self.u_opt[:-1, :], u_of_t(grid)))
            self.x_opt = np.concatenate((self.x_opt, x_of_t(grid)[1:, :]))
        return interp1d(self.t_opt, self.u_opt, axis=0), interp1d(self.t_opt, self.x_opt, axis=0)

    def save_controller_info(self):
        return {'t_opt': self.t_opt, 'u_opt': self.u_opt, 'z_opt': self.dyn_sys.x_to_zfyf(self.x_opt, zf=True),
                'solve_times': self.solve_times, 'rollout_time': self.N_replan * self.dt}
