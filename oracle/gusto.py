"""Oracle: GuSTO sequential-convex-programming outer loop (test infrastructure only).

Restates sofacontrol/scp/gusto.py:283-487 for a prediscretised nn-TPWL
model (oracle/tpwl.py dict) with the QP of oracle/locp.py.
"""
import numpy as np

from . import locp as olocp
from . import tpwl as otpwl

DEFAULTS = dict(delta0=1e4, omega0=1.0, rho=0.1, beta_fail=0.5, gamma_fail=5.0, epsilon=0.01,
                omega_max=1e10, max_gusto_iters=500, convg_thresh=0.1)  # gusto.py:12-22


def max_step(x, xk, xs):
    """max_k |x_scale (x_k - xbar_k)|_inf: what the trust region bounds."""
    return np.max(np.linalg.norm(xs * (x - xk), np.inf, axis=1))


def is_in_trust_region(x, xk, xs, delta, eps):
    """gusto.py:174-183."""
    md = max_step(x, xk, xs)
    return (md, False) if md - delta > eps else (0.0, True)


def mean_step(dsum, N, n):
    """The convergence measure from dsum = sum_k |x_scale (x_k - xbar_k)|_2 (gusto.py:159)."""
    return (1. / N) * (1. / n) * dsum


def is_converged(x, xk, xs, N, thresh):
    """gusto.py:150-161."""
    dsol = mean_step(np.sum(np.linalg.norm(xs * (x - xk), axis=1)), N, x.shape[1])
    return dsol, dsol <= thresh


def start(par):
    """State of the step rule in front of the first QP (gusto.py:320-331)."""
    return dict(delta=par['delta0'], omega=par['omega0'], J_prev=np.inf, d_prev=np.inf, o_prev=np.inf, converged=False)


def running(par, st, itr):
    """gusto.py:333 (is_valid_iteration: gusto.py:163-172)."""
    return itr <= par['max_gusto_iters'] and not st['converged'] and st['omega'] <= par['omega_max']


def judge(par, st, itr, md, J, rho_k, viol, dsol):
    """One transition of the step rule after QP number `itr` (gusto.py:371-428): what becomes of delta, omega, the previous accepted
    (J, delta, omega) and `converged` in `st`.  md = max_step of the QP's minimiser, J its objective; rho_k, viol, dsol: callables for the
    model-accuracy ratio, the largest state-constraint violation and the convergence measure, evaluated only where the rule gets to them.
    Returns (new_solution, tr_ok, rho_k)."""
    if md - st['delta'] > par['epsilon']:
        st['omega'] = par['gamma_fail'] * st['omega']
        return False, False, -1.0
    rho = rho_k()
    if rho > par['rho'] and itr != 1:
        st['delta'] = par['beta_fail'] * st['delta']
        return False, True, rho
    if st['d_prev'] == st['delta'] and st['o_prev'] == st['omega'] and st['J_prev'] <= J:
        st['delta'] = par['beta_fail'] * st['delta']
    st['d_prev'], st['J_prev'], st['o_prev'] = st['delta'], J, st['omega']
    X_ok = not (viol() > par['epsilon'])
    if not X_ok:
        st['omega'] = par['gamma_fail'] * st['omega']
    st['converged'] = bool(dsol() <= par['convg_thresh']) and X_ok
    return True, True, rho


def exit_status(par, st, itr):
    """How a loop that ran out of QPs to try ended (gusto.py:475-483; the kernels' status word): 2 = omega > omega_max, 3 = max
    iterations, else 0."""
    if st['omega'] > par['omega_max']:
        return 2
    return 3 if itr - 1 > par['max_gusto_iters'] else 0


def state_violation(X, x):
    """gusto.py:185-201 with utils.py:394-398 -- all rows k=0..N are checked."""
    if X is None:
        return 0.0
    A, b = X
    return float(max(np.linalg.norm(np.maximum(A @ x[i] - b, 0)) for i in range(x.shape[0])))


def compute_accuracy(model, x, u, xk, uk, J, dt, fs):
    """gusto.py:203-223 with continuous-time nearest-point dynamics (scp/models/tpwl.py:32-50);
    `model` may also be a callable (x, u) -> (f, A, B) (TemplateModel.get_continuous_dynamics)."""
    cont = model if callable(model) else (lambda xx, uu: otpwl.continuous_dynamics(model, xx, uu))
    err = approx = 0.0
    for i in range(x.shape[0] - 1):
        fk, Ak, Bk = cont(xk[i], uk[i])
        f, _, _ = cont(x[i], u[i])
        fa = fk + Ak @ (x[i] - xk[i]) + Bk @ (u[i] - uk[i])
        err += dt * np.linalg.norm(fs * (f - fa), 2)
        approx += dt * np.linalg.norm(fs * fa, 2)
    return err / (J + approx)


def traj_dynamics(model, Ad, Bd, dd, x):
    """gusto.py:225-238 -- table gather at the nearest point of x_k, k=0..N-1."""
    idx = otpwl.nearest_points(model, x[:-1])
    return Ad[idx], Bd[idx], dd[idx], idx


def solve(model, Ad, Bd, dd, H, N, dt, Qz, R, x0, u_init, x_init, z=None, u_des=None, Qzf=None,
          zf=None, U=None, X=None, Xf=None, dU=None, x_char=None, f_char=None, qp_solver=None,
          **kw):
    """One GuSTO.solve call.  Returns xopt, uopt, zopt and a per-iteration trace of
    (J, delta, omega, rho_k, accepted, tr_ok) tuples."""
    def get_traj(xk, uk):
        return traj_dynamics(model, Ad, Bd, dd, xk)[:3]
    return _loop(get_traj, model, H, N, dt, Qz, R, x0, u_init, x_init, z, u_des, Qzf, zf, U, X, Xf, dU, x_char,
                 f_char, qp_solver, kw)


def solve_generic(dyn_d, dyn_c, H, N, dt, Qz, R, x0, u_init, x_init, z=None, u_des=None, Qzf=None, zf=None,
                  U=None, X=None, Xf=None, dU=None, x_char=None, f_char=None, qp_solver=None, obs_lin=None, **kw):
    """The same loop for a generic TemplateModel: dyn_d(x, u) -> (A_d, B_d, d_d)
    (get_discrete_dynamics, gusto.py:225-238), dyn_c(x, u) -> (f, A, B) (get_continuous_dynamics);
    obs_lin(x) -> (H_d, c_d) for models with a nonlinear observer (gusto.py:240-251, 306-310, 467-471)."""
    def get_traj(xk, uk):
        A, B, d = zip(*[dyn_d(xk[i], uk[i]) for i in range(xk.shape[0] - 1)])
        return np.stack(A), np.stack(B), np.stack(d)
    return _loop(get_traj, dyn_c, H, N, dt, Qz, R, x0, u_init, x_init, z, u_des, Qzf, zf, U, X, Xf, dU, x_char,
                 f_char, qp_solver, kw, obs_lin)


def _loop(get_traj, model, H, N, dt, Qz, R, x0, u_init, x_init, z, u_des, Qzf, zf, U, X, Xf, dU, x_char, f_char,
          qp_solver, kw, obs_lin=None):
    par = dict(DEFAULTS); par.update(kw)

    def get_obs(xk):
        if obs_lin is None:
            return None, None
        Hs, cs = zip(*[obs_lin(xk[i]) for i in range(xk.shape[0])])
        return np.stack(Hs), np.stack(cs)
    n = x0.shape[0]
    xs = 1. / np.abs(x_char) if x_char is not None else np.ones(n)
    fs = 1. / np.abs(f_char) if f_char is not None else np.ones(n)
    stage_qp = isinstance(qp_solver, str) and qp_solver == 'riccati_ipm'
    cond_qp = isinstance(qp_solver, str) and qp_solver == 'condensed_ipm'
    if qp_solver is None:
        def qp_solver(qp):
            w, _, _ = olocp.solve_exact(qp)
            return w
    xk, uk = x_init.copy(), u_init.copy()
    A_k, B_k, d_k = get_traj(xk, uk)
    H_k, c_k = get_obs(xk)
    st = start(par)
    itr = 0
    trace = []
    warm_state, ipm_iters = None, []
    while running(par, st, itr):
        delta, omega = st['delta'], st['omega']
        if stage_qp:
            # the stage-structured interior point (numpy statement of the kernel's algorithm) on the same QP data;
            # seconds instead of minutes at the BASELINE shapes.  Checked against solve_exact in tests/test_locp_oracle.py
            from . import riccati_ipm as ripm
            assert dU is None and obs_lin is None
            sp = ripm.Problem(N, H, Qz, R, A_k, B_k, d_k, x0, xk, delta, omega, z=z, u_des=u_des, Qzf=Qzf, zf=zf,
                              U=U, X=X, Xf=Xf, x_scale=xs)
            x_next, u_next, _, J, _ = ripm.solve(sp)
        elif cond_qp:
            # the condensed interior point (numpy statement of csrc/locp_cond.h) with the kernel's control flow: the QP
            # without its trust-region rows first; the full stage-structured solve only if that minimiser leaves the
            # trust region
            from . import riccati_ipm as ripm, condensed_ipm as cipm
            assert dU is None and obs_lin is None
            sp = ripm.Problem(N, H, Qz, R, A_k, B_k, d_k, x0, xk, delta, omega, z=z, u_des=u_des, Qzf=Qzf, zf=zf,
                              U=U, X=X, Xf=Xf, x_scale=xs)
            # (round 4) every QP after the first one the condensed path finished starts from that one's iterate
            x_next, u_next, J, info = cipm.solve(sp, warm=warm_state if par.get('warm_start_qp', True) else None)
            J += omega * max(0.0, np.max(np.abs(xs * (x0 - xk[0]))) - delta)       # s_0 (closed form)
            ipm_iters.append(info['iters'])
            if info['status'] == 'optimal':
                warm_state = info['final']
            if not (info['status'] == 'optimal' and info['inside']):
                x_next, u_next, _, J, _ = ripm.solve(sp)
        else:
            qp = olocp.build_qp(N, H, Qz, R, A_k, B_k, d_k, x0, xk, delta, omega, z=z, u_des=u_des,
                                Qzf=Qzf, zf=zf, U=U, X=X, Xf=Xf, dU=dU, x_scale=xs, Hd=H_k, cd=c_k)
            if par.get('input_nullspace') is not None:
                # locp.py:258-261: the objective (and with it the J of the accuracy ratio, gusto.py:405-420) carries the term
                w, J, _ = olocp.solve_with_nullspace(qp, par['input_nullspace'])
            else:
                w = qp_solver(qp)
                J = olocp.objective(qp, w)
            x_next, u_next, _ = olocp.split(qp, w)
        new_solution, tr_ok, rho_k = judge(
            par, st, itr, max_step(x_next, xk, xs), J,
            rho_k=lambda: compute_accuracy(model, x_next, u_next, xk, uk, J, dt, fs),
            viol=lambda: state_violation(X, x_next),
            dsol=lambda: is_converged(x_next, xk, xs, N, par['convg_thresh'])[0])
        itr += 1
        trace.append((J, delta, omega, rho_k, new_solution, tr_ok))
        if new_solution:
            xk, uk = x_next.copy(), u_next.copy()
            if par['max_gusto_iters'] >= 1:
                A_k, B_k, d_k = get_traj(xk, uk)
                H_k, c_k = get_obs(xk)
    zopt = (H @ xk.T).T
    return xk, uk, zopt, trace
