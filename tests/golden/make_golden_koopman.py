"""Golden vectors of the Koopman baseline, by IMPORTING THE REFERENCE (build container only).

Usage:  python tests/golden/make_golden_koopman.py          (writes tests/golden/g22_koopman.npz)

Imports sofacontrol.baselines.koopman through the stand-in modules of _ref_import.py.  Stores the shipped diamond model
(examples/diamond/koopman_model.mat) as plain arrays, the reference's observable orders, scalings, get_zeta /
add_zeta_offline, lift_data, and a KoopmanMPC.evaluate trace whose MPC client is a stub that records every request and
answers with oracle.locp.solve_exact on the constant-model QP.  The GPU box never runs this script.
"""
import io
import os
import sys
import contextlib

import numpy as np
import sympy as sp
from scipy.interpolate import interp1d
from scipy.io import loadmat
from sympy.polys.monomials import itermonomials
from sympy.polys.orderings import monomial_key

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import _ref_import  # noqa: E402

_ref_import.install()

from sofacontrol.baselines.koopman import koopman_utils as rku  # noqa: E402
from sofacontrol.baselines.koopman import koopman as rk  # noqa: E402

from oracle import locp as olocp  # noqa: E402

MAT = os.path.join(_ref_import.REF, 'examples', 'diamond', 'koopman_model.mat')


def order(nz, deg, dmd):
    """Exponent rows of get_lifting_function's list (koopman_utils.py:162-172)."""
    zeta = sp.symbols('zeta1:{}'.format(nz + 1))
    polys = sorted(itermonomials(list(zeta), deg), key=monomial_key('grlex', list(reversed(zeta))))
    if dmd:
        polys = polys[1:]
    else:
        polys.append(polys[0])
        polys = polys[1:]
    return np.array([sp.Poly(p, *zeta).monoms()[0] if p != 1 else (0,) * nz for p in polys], dtype=np.int32)


def diamond_cost(model, scaling, N):
    """diamond_koopman.py:146-185 (cost, U box, target), as plain arrays."""
    T = 10
    t = np.linspace(0, T, 1000)
    th = np.linspace(0, 2 * np.pi, 1000)
    zt = np.zeros((1000, model.n))
    zt[:, 0] = -15. * np.sin(th)
    zt[:, 1] = 15. * np.sin(2 * th)
    zt[:, 2] -= 114
    z_norm = scaling.scale_down(y=zt)
    u_norm = scaling.scale_down(u=np.zeros(model.m)).reshape(-1)
    R = .00001 * np.eye(model.m)
    Q = np.zeros((model.n, model.n))
    Q[0, 0] = 100
    Q[1, 1] = 100
    R *= np.diag(scaling.u_factor[0])
    Q *= np.diag(scaling.y_factor[0])
    ub = scaling.scale_down(u=1500. * np.ones(model.m)).reshape(-1)
    lb = scaling.scale_down(u=200. * np.ones(model.m)).reshape(-1)
    UA = np.vstack([np.eye(model.m), -np.eye(model.m)])
    Ub = np.concatenate([ub, -lb])
    return dict(t=t, z=z_norm, u=u_norm, Q=Q, R=R, UA=UA, Ub=Ub)


class StubClient:
    """MPCClientNode stand-in: records every send_request(t, x0), answers with the exact QP (no trust region, constant A, B)."""
    requests = []

    def __init__(self):
        self.sol = None

    def send_request(self, t0, x0, wait=True):
        g = self.cfg
        StubClient.requests.append((float(t0), np.asarray(x0, dtype=float).copy()))
        N, dt = g['N'], g['Ts']
        t = t0 + dt * np.arange(N + 1)
        zi = interp1d(g['t'], g['z'], axis=0, bounds_error=False, fill_value=(g['z'][0], g['z'][-1]))
        z = zi(t)
        u_des = np.tile(g['u'].reshape(1, -1), (N, 1))
        A, B = g['A'], g['B']
        qp = olocp.build_qp(N, g['H'], g['Q'], g['R'], [A] * N, [B] * N, [np.zeros(A.shape[0])] * N, np.asarray(x0, float),
                            None, 0.0, 0.0, z=z, u_des=u_des, U=(g['UA'], g['Ub']), tr_active=False)
        w, _, _ = olocp.solve_exact(qp)
        x, u, _ = olocp.split(qp, w)
        self.sol = (t, u, x)

    def force_spin(self):
        pass

    def check_if_done(self):
        return True

    def force_wait(self):
        pass

    def get_solution(self, n_x, n_u):
        t, u, x = self.sol
        return t, u, x, 0.0


def main(out):
    res = {}
    raw = loadmat(MAT)['py_data'][0, 0]
    rm, rp = raw['model'], raw['params']
    model = rku.KoopmanModel(rm, rp)
    for k in ('A', 'B', 'C', 'M', 'K'):
        res['model_' + k] = np.asarray(rm[k][0, 0], dtype=np.float64)
    for k in ('n', 'm', 'N', 'nzeta', 'delays', 'obs_degree'):
        res['param_' + k] = np.array(int(rp[k]))
    res['param_Ts'] = np.array(float(rp['Ts']))
    res['param_obs_type'] = np.array(str(rp['obs_type'][0, 0][0, 0][0]))
    sc = model.scale
    for k in ('y_offset', 'y_factor', 'u_offset', 'u_factor'):
        res['scale_' + k] = np.asarray(sc[k][0, 0], dtype=np.float64)
    # observable orders
    for nz, deg in ((10, 2), (3, 3), (4, 4)):
        for dmd in (0, 1):
            res['order_%d_%d_%d' % (nz, deg, dmd)] = order(nz, deg, dmd)
    # scaling
    rng = np.random.default_rng(220)
    scaling = rku.KoopmanScaling(sc)
    ys = res['scale_y_offset'] + 20 * rng.standard_normal((5, 3))
    us = 200 + 1300 * rng.random((5, 4))
    res['scal_y'], res['scal_u'] = ys, us
    res['scal_y_down'] = scaling.scale_down(y=ys)
    res['scal_u_down'] = scaling.scale_down(u=us)
    res['scal_y_up'] = scaling.scale_up(y=ys)
    res['scal_u_up'] = scaling.scale_up(u=us)
    res['scal_y1_down'] = scaling.scale_down(y=ys[0])      # 1-D input: (1, n) result
    # get_zeta over a record, delays 1..3
    T = 9
    Yr = res['scale_y_offset'] + 10 * rng.standard_normal((T, 3))
    Ur = 200 + 1300 * rng.random((T, 4))
    res['rec_y'], res['rec_u'] = Yr, Ur
    for d in (1, 2, 3):
        kd = rku.KoopmanData(sc, d)
        zs, ok = [], []
        for i in range(T):
            kd.add_measurement(Yr[i], Ur[i])
            z = kd.get_zeta()
            ok.append(z is not None)
            zs.append(np.full(3 * (d + 1) + 4 * d, np.nan) if z is None else z)
        res['zeta_online_%d' % d] = np.stack(zs)
        res['zeta_online_ok_%d' % d] = np.array(ok)
        res['ynorm_shape_%d' % d] = np.array(kd.y_norm.shape)
        ko = rku.KoopmanOfflineData(sc, d)
        ko.y_norm = ko.scaling.scale_down(y=Yr)
        ko.u_norm = ko.scaling.scale_down(u=Ur)
        ko.add_zeta_offline()
        res['zeta_offline_%d' % d] = ko.zeta
    # lift_data of the delay-1 zetas (the shipped model), with and without DMD
    Z = res['zeta_offline_1']
    res['lift'] = np.array([np.asarray(model.lift_data(*z), dtype=float) for z in Z])
    model_dmd = rku.KoopmanModel(rm, rp, DMD=True)
    res['lift_dmd'] = np.array([np.asarray(model_dmd.lift_data(*z), dtype=float) for z in Z])
    # KoopmanMPC.evaluate traces: sim dt 0.01, Ts 0.05, t_delay 2, N 5, rollout 1 / 3, input_hold off / on
    N = 5
    cost = diamond_cost(model, scaling, N)
    for k, v in cost.items():
        res['cost_' + k] = v
    res['mpc_N'] = np.array(N)
    cfg = dict(cost, N=N, Ts=model.Ts, H=model.H, A=model.A_d, B=model.B_d)
    StubClient.cfg = cfg
    rk.MPCClientNode = StubClient
    steps = 260
    t_sim = 0.01 * np.arange(steps)
    y_meas = res['scale_y_offset'][0] + np.stack([3 * np.sin(2 * t_sim), 2 * np.cos(3 * t_sim), 0.5 * np.sin(t_sim)], axis=1)
    res['trace_y'] = y_meas
    for rh in (1, 3):
        for hold in (0, 1):
            StubClient.requests = []
            c = rk.KoopmanMPC(model, delay=2, u0=np.full(model.m, 300.), rollout_horizon=rh, input_hold=bool(hold))
            c.set_sim_timestep(0.01)
            us = []
            u_prev = np.full(model.m, 300.)
            with contextlib.redirect_stdout(io.StringIO()):
                for k in range(steps):
                    u_prev = c.evaluate(t_sim[k], y_meas[k], None, u_prev)
                    us.append(u_prev)
            info = c.save_controller_info()
            tag = 'tr_%d_%d_' % (rh, hold)
            res[tag + 'u'] = np.stack(us)
            res[tag + 'req_t'] = np.array([r[0] for r in StubClient.requests])
            res[tag + 'req_x0'] = np.stack([r[1] for r in StubClient.requests])
            for k in ('t_opt', 'u_opt', 'z_opt', 'zopt_full'):
                res[tag + k] = np.asarray(info[k])
            res[tag + 'z_rollout'] = np.stack(info['z_rollout'])
            res[tag + 't_rollout'] = np.stack(info['t_rollout'])
            res[tag + 'n_solves'] = np.array(len(info['solve_times']))
            res[tag + 'rollout_time'] = np.array(info['rollout_time'])
    np.savez_compressed(os.path.join(out, 'g22_koopman.npz'), **res)


if __name__ == '__main__':
    main(HERE)
