"""Generate tests/golden/g25_ilqr_loop.npz by IMPORTING THE REFERENCE (build container only).

Usage:  python tests/golden/make_golden_ilqr_loop.py

The reference's tpwl.controllers.ilqr on the g8 problem (r = 4, m = 3, P = 7, pre-discretised at dt = 0.05, trajectory target, N = 12),
closed on the reference's own TPWL model stepped at dt_sim = 0.01 -- every simulation step goes through controller.evaluate -- once with
the FullStateObserver and once with a DiscreteEKFObserver on six measured coordinates, with seeded disturbances and measurement noise.
At dt = 0.05 the controller steps 3, 6, 7 read the policy rows 2, 5, 6; step 13 (t_step = 0.65 > final_time = 0.61) returns u0, and the
trace ends there (a longer final_time would reach row == N, where the reference raises IndexError).

Stored (data only): the reduced plant states, u, the beliefs x_hat, the measurements y, the policy x_bar, u_bar, K, the noise used, the
reference's own discrete tables at dt and dt_sim, the filter's covariances and its covariance behind the first update.  The evaluate
calls are handed the reduced state through a pass-through ROM (compute_RO_state returns what it is given), so the belief of the
FullStateObserver is the plant state bit for bit and the trace holds no lift / project rounding."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (installs the stand-ins and imports the reference)

from sofacontrol import utils as rutils  # noqa: E402
from sofacontrol.tpwl.tpwl_utils import Target  # noqa: E402
import sofacontrol.tpwl.controllers as ctl  # noqa: E402
from sofacontrol.tpwl.observer import DiscreteEKFObserver  # noqa: E402

DT, DT_SIM, R_STEPS, STEPS = 0.05, 0.01, 5, 70
FINAL_TIME = 0.61                      # int(0.61 / 0.05) = 12 = N (0.6 / 0.05 rounds below 12)
MEAS_NODES = [3, 9]


class PassThroughRom:
    """The controller's ROM during the trace: evaluate is handed the reduced state itself."""

    def __init__(self, rom):
        self.V, self.x_ref = rom.V, rom.x_ref

    def compute_RO_state(self, xf=None, **kw):
        return np.asarray(xf).copy()


def tables(tp, dt):
    d = tp.tpwl_dict
    out = [tp.discretize_dynamics(d['A_c'][i], d['B_c'][i], d['d_c'][i], dt) for i in range(len(d['q']))]
    return [np.stack([o[k] for o in out]) for k in range(3)]


def trace(tp, ctrl, x0, w, v, C, y_ref):
    """STEPS simulation steps: y_s = C x_s + y_ref + v_s, u_s = evaluate(t_s, y_s, x_s, u_{s-1}), x_{s+1} = plant(x_s, u_s) + w_s."""
    m = tp.get_input_dim()
    x, u_prev = x0.copy(), np.zeros(m)
    X, U, XH, Y = [x0.copy()], [], [], []
    sigma_first = None
    for s in range(STEPS):
        y = np.asarray(C @ x).ravel() + y_ref + (v[s] if v is not None else 0.0)
        u = ctrl.evaluate(s * DT_SIM, y, x, u_prev)
        if s == 0 and hasattr(ctrl.observer, 'Sigma'):
            sigma_first = np.asarray(ctrl.observer.Sigma).copy()
        XH.append(np.asarray(ctrl.observer.x).copy()); U.append(u.copy()); Y.append(y)
        A, B, d = tp.get_jacobians(x, DT_SIM)
        x = tp.update_dynamics(x, u, A, B, d)
        if w is not None:
            x = x + w[s]
        X.append(x.copy())
        u_prev = u
    return np.stack(X), np.stack(U), np.stack(XH), np.stack(Y), sigma_first


def main():
    r, m, P, n_nodes = 4, 3, 7, 20
    model, U, q_ref, v_ref, Hf = mg.make_problem(r, m, P, n_nodes, 40, q_scale=0.05)
    Cf = mg.meas_selector(MEAS_NODES, n_nodes)
    n = 2 * r
    rng = np.random.default_rng(2500)
    tgt = Target()
    tgt.t = np.linspace(0, FINAL_TIME, 31)
    cost = rutils.QuadraticCost(Q=np.diag([0, 0, 0, 100., 100., 0]), R=1e-3 * np.eye(m), Qf=np.diag([0, 0, 0, 100., 100., 0]))
    u0 = np.array([5.0, 10.0, 15.0])
    x0 = 1e-3 * rng.standard_normal(n)
    w = 1e-5 * rng.standard_normal((STEPS, n))
    v = 1e-3 * rng.standard_normal((STEPS, 3 * len(MEAS_NODES)))
    G = rng.standard_normal((n, n))
    Wf = 10 * np.eye(n) + 0.1 * (G + G.T)
    Vf = 0.1 * np.eye(6) + 0.01 * np.diag(rng.uniform(0, 1, 6))
    Sigma0 = 0.5 * np.eye(n)
    res = dict(dt=DT, dt_sim=DT_SIM, final_time=FINAL_TIME, u0=u0, x0=x0, w=w, v=v, Wf=Wf, Vf=Vf, Sigma0=Sigma0, Cf=Cf.toarray(),
               meas_nodes=np.array(MEAS_NODES))
    for tag in ('full', 'ekf'):
        tp = mg.rtpwl.TPWLATV(data=dict(q=model['q'], v=model['v'], u=model['u'], A_c=model['A_c'], B_c=model['B_c'], d_c=model['d_c'],
                                        rom_info=dict(type='POD', U=U, q_ref=q_ref, v_ref=v_ref)),
                              params=dict(tpwl_method='nn', dist_weights={'q': model['w_q'], 'v': model['w_v']}, beta_weighting=None),
                              Cf=Cf, Hf=Hf, discr_method='zoh')
        mg.quiet(tp.pre_discretize, DT)
        tgt.z = np.zeros((31, 6)); tgt.z[:, 3] = -1.0 * np.sin(10 * tgt.t); tgt.z[:, 4] = 0.5 * np.sin(20 * tgt.t)
        tgt.z = tgt.z + np.asarray(tp.z_ref)
        tgt.Hf = Hf
        obs = DiscreteEKFObserver(tp, Sigma0=Sigma0.copy(), W=Wf, V=Vf) if tag == 'ekf' else None
        (ctrl, _) = mg.quiet(ctl.ilqr, tp, cost, tgt, dt=DT, observer=obs, delay=0.0, u0=u0)
        ctrl.set_sim_timestep(DT_SIM)
        assert ctrl.planning_horizon == 12
        C, y_ref = np.asarray(tp.C), np.asarray(tp.y_ref).ravel()
        tp.rom = PassThroughRom(tp.rom)
        (out, _) = mg.quiet(trace, tp, ctrl, x0, w if tag == 'ekf' else None, v if tag == 'ekf' else None, C, y_ref)
        X, Us, XH, Y, sigma_first = out
        for k, a in (('x', X), ('u', Us), ('x_hat', XH), ('y', Y), ('x_bar', ctrl.x_bar), ('u_bar', ctrl.u_bar), ('K', np.stack(ctrl.K))):
            res['%s_%s' % (tag, k)] = np.asarray(a)
        if tag == 'ekf':
            res['ekf_Sigma_first'] = sigma_first
        res['z_target'] = np.asarray(ctrl.policy.z_target)
    Ad, Bd, dd = tables(tp, DT)
    As, Bs, ds = tables(tp, DT_SIM)
    res.update(Ad=Ad, Bd=Bd, dd=dd, Ad_sim=As, Bd_sim=Bs, dd_sim=ds, C=C, y_ref=y_ref, H=np.asarray(tp.H), z_ref=np.asarray(tp.z_ref))
    path = os.path.join(HERE, 'g25_ilqr_loop.npz')
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path))
    print('idle tail from step', int(np.argmax((res['full_u'] == u0).all(axis=1))), 'full-state |x| max', float(np.abs(res['full_x']).max()))


if __name__ == '__main__':
    main()
