"""Golden vectors of the ROMPC baseline, by IMPORTING THE REFERENCE (build container only).

Usage:  python tests/golden/make_golden_rompc.py          (writes tests/golden/g23_rompc.npz)

Imports sofacontrol.baselines.rompc through the stand-in modules of _ref_import.py.  The model is point 0 of the synthetic
TPWL tables of make_golden.make_problem(4, 3, 3, 20, 230); Cf is the reference's MeasurementModel over five nodes (30 rows:
the observer's DARE has 30 "inputs"), Hf its tip linearModel.  Stores LinearROM's attributes and conversions, both gains,
observer-only traces (with and without an output model), two ROMPC.evaluate traces whose MPC client is a stub that records
every request and answers with oracle.locp.solve_exact on the constant-model QP, and a TPWL2LinearROM round trip.  The GPU
box never runs this script.
"""
import io
import os
import sys
import tempfile
import contextlib

import numpy as np
from scipy.interpolate import interp1d

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import _ref_import  # noqa: E402

_ref_import.install()

import make_golden as mg  # noqa: E402
from sofacontrol.baselines.rompc import rompc_utils as rru  # noqa: E402
from sofacontrol.baselines.rompc import observer as robs  # noqa: E402
from sofacontrol.baselines.rompc import rompc as rr  # noqa: E402
from sofacontrol.measurement_models import MeasurementModel, linearModel  # noqa: E402
from sofacontrol.utils import QuadraticCost, save_data, load_data  # noqa: E402

from oracle import locp as olocp  # noqa: E402

NODES = [1, 5, 9, 13, 17]
N_NODES = 20


class StubClient:
    """MPCClientNode stand-in: records every send_request(t, x0), answers with the exact QP (no trust region, constant
    A, B, d over the horizon)."""
    requests = []
    solves = []
    cfg = None

    def __init__(self):
        self.sol = None

    def send_request(self, t0, x0, wait=True):
        g = StubClient.cfg
        StubClient.requests.append((float(t0), np.asarray(x0, dtype=float).copy()))
        N, dt = g['N'], g['dt']
        t = t0 + dt * np.arange(N + 1)
        z = interp1d(g['t'], g['z'], axis=0, bounds_error=False, fill_value=(g['z'][0], g['z'][-1]))(t)
        A, B, d = g['A'], g['B'], g['d']
        qp = olocp.build_qp(N, g['H'], g['Q'], g['R'], [A] * N, [B] * N, [d] * N, np.asarray(x0, float), None, 0.0, 0.0, z=z,
                            U=(g['UA'], g['Ub']), tr_active=False)
        w, _, _ = olocp.solve_exact(qp)
        x, u, _ = olocp.split(qp, w)
        StubClient.solves.append(u.copy())
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


def plant_record(rom_model, steps, seed, u_amp):
    """A deterministic full-order record to drive the controller with: the reduced model itself under a smooth input,
    plus a small perturbation, lifted by the basis.  Returns xf (steps x 2 n_f), u (steps x m)."""
    rng = np.random.default_rng(seed)
    n, m = rom_model.state_dim, rom_model.input_dim
    x = 0.02 * rng.standard_normal(n)
    ph = rng.uniform(0, 2 * np.pi, m)
    xs, us = [], []
    for k in range(steps):
        u = u_amp * (1.0 + np.sin(0.3 * k + ph))
        xs.append(x.copy()); us.append(u)
        x = rom_model.update_state(x, u) + 1e-4 * rng.standard_normal(n)
    xs = np.stack(xs)
    xf = xs @ rom_model.rom.V.T + rom_model.rom.x_ref
    return xf, np.stack(us)


def run_trace(model, cost, costL, dt, N_replan, delay, steps, xf, Cf, tag, res):
    StubClient.requests, StubClient.solves = [], []
    c = rr.ROMPC(model, cost, costL, dt, N_replan=N_replan, delay=delay)
    us, xs, zs = [], [], []
    u_prev = np.zeros(model.input_dim)
    with contextlib.redirect_stdout(io.StringIO()):
        for k in range(steps):
            y = Cf @ xf[k]
            u_prev = c.evaluate(dt * k, y, xf[k], u_prev)
            us.append(u_prev); xs.append(c.observer.x.copy()); zs.append(np.array(c.observer.z).copy())
    info = c.save_controller_info()
    res[tag + 'u'] = np.stack(us)
    res[tag + 'xhat'] = np.stack(xs)
    res[tag + 'z'] = np.stack(zs)
    res[tag + 'req_t'] = np.array([r[0] for r in StubClient.requests])
    res[tag + 'req_x0'] = np.stack([r[1] for r in StubClient.requests])
    for k in ('t_opt', 'u_opt', 'z_opt'):
        res[tag + k] = np.asarray(info[k])
    res[tag + 'x_opt'] = c.x_opt
    res[tag + 'n_solves'] = np.array(len(info['solve_times']))
    res[tag + 'rollout_time'] = np.array(info['rollout_time'])
    res[tag + 'steps'] = np.array(steps)
    res[tag + 'dt'] = np.array(dt)
    res[tag + 'delay'] = np.array(delay)
    res[tag + 'N_replan'] = np.array(N_replan)
    return c, np.concatenate(StubClient.solves)


def main(out):
    res = {}
    tp_model, U, q_ref, v_ref, Hf = mg.make_problem(4, 3, 3, N_NODES, 230)
    for k, v in tp_model.items():
        res['model_' + k] = np.asarray(v)
    res['U'], res['q_ref'], res['v_ref'] = U, q_ref, v_ref
    rom_info = dict(type='POD', U=U, q_ref=q_ref, v_ref=v_ref)
    data = dict(A_c=tp_model['A_c'][0], B_c=tp_model['B_c'][0], d_c=tp_model['d_c'][0], rom_info=rom_info)
    Cf = MeasurementModel(NODES, N_NODES).C
    res['Cf'] = np.asarray(Cf.todense())
    res['Hf'] = np.asarray(Hf.todense())
    res['nodes'] = np.array(NODES)
    dt, dt_mpc = 0.01, 0.05
    model = rru.LinearROM(data, dt, Cf=Cf, Hf=Hf)
    model_noH = rru.LinearROM(data, dt, Cf=Cf)
    model_mpc = rru.LinearROM(data, dt_mpc, Cf=Cf, Hf=Hf)
    res['dt'], res['dt_mpc'] = np.array(dt), np.array(dt_mpc)
    for k in ('A_d', 'B_d', 'd_d', 'C', 'y_ref', 'H', 'z_ref'):
        res['rom_' + k] = np.asarray(getattr(model, k))
        res['mpc_' + k] = np.asarray(getattr(model_mpc, k))
    for k in ('state_dim', 'N', 'input_dim', 'meas_dim', 'output_dim'):
        res['rom_' + k] = np.array(getattr(model, k))
    # conversions on a few points
    rng = np.random.default_rng(231)
    X = 0.05 * rng.standard_normal((4, model.state_dim))
    res['conv_x'] = X
    res['conv_zf'] = model.x_to_zfyf(X, zf=True)
    res['conv_yf'] = model.x_to_zfyf(X, yf=True)
    res['conv_z'] = model.x_to_zy(X, z=True)
    res['conv_x1_zf'] = model.x_to_zfyf(X[0], zf=True)
    res['conv_zf_to_z'] = model.zfyf_to_zy(zf=res['conv_zf'])
    res['conv_yf_to_y'] = model.zfyf_to_zy(yf=res['conv_yf'])
    res['conv_z_to_zf'] = model.zy_to_zfyf(z=res['conv_z'])
    res['conv_y_to_yf'] = model.zy_to_zfyf(y=res['conv_yf_to_y'])
    res['conv_noH_yf'] = model_noH.x_to_zfyf(X, yf=True)
    res['conv_update_state'] = np.stack([model.update_state(x, np.array([100., 200., 300.])) for x in X])
    # costs (diamond_rompc.py:67-77) and gains
    Qz = np.diag([0., 0., 0., 100., 100., 0.])
    cost = QuadraticCost(); cost.Q = model.H.T @ Qz @ model.H; cost.R = 1e-4 * np.eye(model.input_dim)
    costL = QuadraticCost(); costL.Q = cost.Q; costL.R = 1e-3 * np.eye(model.meas_dim)
    res['Qz'], res['cost_Q'], res['cost_R'], res['costL_R'] = Qz, cost.Q, cost.R, costL.R
    import sofacontrol.lqr.lqr as rlqr
    K, PK = rlqr.dare(model.A_d, model.B_d, cost.Q, cost.R)
    Lg, PL = rlqr.dare(model.A_d.T, model.C.T, costL.Q, costL.R)
    res['K'], res['PK'], res['L'], res['PL'] = K, PK, -Lg.T, PL
    rho = lambda M: float(np.abs(np.linalg.eigvals(M)).max())
    res['rho'] = np.array([rho(model.A_d), rho(model.A_d - res['L'] @ model.C), rho(model.A_d + model.B_d @ K)])
    # hardware configuration: controller at the MPC's time step
    cost_hw = QuadraticCost(); cost_hw.Q = model_mpc.H.T @ Qz @ model_mpc.H; cost_hw.R = cost.R
    costL_hw = QuadraticCost(); costL_hw.Q = cost_hw.Q; costL_hw.R = costL.R
    K_hw, _ = rlqr.dare(model_mpc.A_d, model_mpc.B_d, cost_hw.Q, cost_hw.R)
    L_hw, _ = rlqr.dare(model_mpc.A_d.T, model_mpc.C.T, costL_hw.Q, costL_hw.R)
    res['K_hw'], res['L_hw'] = K_hw, -L_hw.T
    # observer-only traces: initialize, then updates, with and without an output model
    steps_obs = 25
    xf, u_rec = plant_record(model, steps_obs, 232, 150.0)
    res['obs_xf0'] = xf[0]
    res['obs_u'] = u_rec
    res['obs_yf'] = (Cf @ xf.T).T
    for tag, mdl in (('obs_H_', model), ('obs_noH_', model_noH)):
        ob = robs.DiscreteLuenbergerObserver(mdl, costL.Q, costL.R)
        ob.initialize(xf[0])
        xs, zs = [ob.x.copy()], [np.array(ob.z).copy()]
        for k in range(steps_obs):
            ob.update(u_rec[k], res['obs_yf'][k])
            xs.append(ob.x.copy()); zs.append(np.array(ob.z).copy())
        res[tag + 'x'], res[tag + 'z'] = np.stack(xs), np.stack(zs)
    # ROMPC traces.  The QP of the stub: MPC model at dt_mpc, N = 5, output cost Qz, R, a slow figure in the reduced outputs
    N = 5
    t_tgt = np.linspace(0, 3, 300)
    z_tgt = np.zeros((300, model.output_dim))
    z_tgt[:, 3] = -0.01 * np.sin(2 * np.pi * t_tgt / 3)
    z_tgt[:, 4] = 0.005 * np.sin(4 * np.pi * t_tgt / 3)
    m = model.input_dim
    UA = np.vstack([np.eye(m), -np.eye(m)])
    cfg = dict(N=N, dt=dt_mpc, H=model_mpc.H, Q=Qz, R=1e-5 * np.eye(m), A=model_mpc.A_d, B=model_mpc.B_d, d=model_mpc.d_d,
               t=t_tgt, z=z_tgt, UA=UA, Ub=np.full(2 * m, 1e9))
    StubClient.cfg = cfg
    rr.MPCClientNode = StubClient
    steps = 48
    xf_tr, _ = plant_record(model, steps, 233, 20.0)
    scratch = {}
    _, u_free = run_trace(model, cost, costL, dt, 10, 0.05, steps, xf_tr, Cf, 'free_', scratch)
    # the U box from the unconstrained run: 60 % of the range it used, so that some recorded solve sits on a bound
    ub, lb = 0.6 * u_free.max(), 0.6 * u_free.min()
    cfg['Ub'] = np.concatenate([np.full(m, ub), np.full(m, -lb)])
    _, u_box = run_trace(model, cost, costL, dt, 10, 0.05, steps, xf_tr, Cf, 'tr_', res)
    active = (np.abs(u_box - ub) < 1e-7 * max(1.0, abs(ub))) | (np.abs(u_box - lb) < 1e-7 * max(1.0, abs(lb)))
    assert active.any(), 'no recorded solve has an active input bound'
    assert len(res['tr_req_t']) >= 6
    res['tr_xf'] = xf_tr
    res['tr_n_active'] = np.array(int(active.sum()))
    steps_hw = 24
    xf_hw, _ = plant_record(model_mpc, steps_hw, 234, 20.0)
    run_trace(model_mpc, cost_hw, costL_hw, dt_mpc, 1, 0.1, steps_hw, xf_hw, Cf, 'hw_', res)
    res['hw_xf'] = xf_hw
    for k in ('N', 'dt', 'Q', 'R', 't', 'z', 'UA', 'Ub'):
        res['qp_' + k] = np.asarray(cfg[k])
    # TPWL2LinearROM through a temporary pickle
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = os.path.join(tmp, 'tpwl.pkl'), os.path.join(tmp, 'lin.pkl')
        save_data(src, dict(tp_model, rom_info=rom_info))
        rru.TPWL2LinearROM(src, dst)
        lin = load_data(dst)
    res['lin_keys'] = np.array(sorted(lin.keys()))
    for k in ('A_c', 'B_c', 'd_c'):
        res['lin_' + k] = np.asarray(lin[k])
    res['lin_rom_U'] = np.asarray(lin['rom_info']['U'])
    res['lin_rom_type'] = np.array(lin['rom_info']['type'])
    np.savez_compressed(os.path.join(out, 'g23_rompc.npz'), **res)
    print('rho(A_d) %.3f  rho(A_d - L C) %.3f  rho(A_d + B K) %.3f; requests at' % tuple(res['rho']), res['tr_req_t'],
          '; active bounds', int(active.sum()), '; U box', lb, ub)


if __name__ == '__main__':
    main(HERE)
