"""CPU: surface of the ROMPC baseline (sofacontrol/baselines/rompc), its C ABI declarations, and TPWL2LinearROM (host I/O)
against the golden vectors of the imported reference (g23)."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_surface_names():
    import sofacontrol_amd.baselines.rompc.rompc_utils as ru
    import sofacontrol_amd.baselines.rompc.observer as ob
    import sofacontrol_amd.baselines.rompc.rompc as rp
    import sofacontrol_amd.lqr.lqr as lqr
    assert hasattr(lqr, 'dare_wide') and hasattr(lqr, 'dare')
    for n in ('LinearROM', 'TPWL2LinearROM'):
        assert hasattr(ru, n)
    for m in ('get_jacobians', 'update_dynamics', 'update_state', 'set_measurement_model', 'set_output_model', 'zfyf_to_zy',
              'zy_to_zfyf', 'x_to_zfyf', 'x_to_zy', 'get_state_dim', 'get_input_dim', 'get_output_dim', 'get_meas_dim',
              'get_rom_info'):
        assert hasattr(ru.LinearROM, m), m
    for m in ('initialize', 'update', 'update_z', 'replay', 'L'):
        assert hasattr(ob.DiscreteLuenbergerObserver, m), m
    assert isinstance(ob.DiscreteLuenbergerObserver.L, property) and ob.DiscreteLuenbergerObserver.L.fset is not None
    for m in ('evaluate', 'solve_OCP', 'get_OCP_solution', 'save_controller_info', 'K'):
        assert hasattr(rp.ROMPC, m), m
    assert isinstance(rp.ROMPC.K, property) and rp.ROMPC.K.fset is not None
    from sofacontrol_amd.closed_loop_controller import TemplateController
    assert issubclass(rp.ROMPC, TemplateController)


def test_update_dynamics_is_the_affine_map():
    from sofacontrol_amd.baselines.rompc.rompc_utils import LinearROM
    rng = np.random.default_rng(0)
    A, B, d = rng.standard_normal((5, 5)), rng.standard_normal((5, 2)), rng.standard_normal(5)
    x, u = rng.standard_normal(5), rng.standard_normal(2)
    np.testing.assert_allclose(LinearROM.update_dynamics(x, u, A, B, d), A @ x + B @ u + d, rtol=0, atol=1e-15)


def test_tpwl2linearrom_against_golden(golden, tmp_path):
    from sofacontrol_amd.baselines.rompc.rompc_utils import TPWL2LinearROM
    from sofacontrol_amd.utils import save_data, load_data
    g = golden('g23_rompc')
    tpwl = {k: g['model_' + k] for k in ('q', 'v', 'u', 'A_c', 'B_c', 'd_c')}
    tpwl['rom_info'] = dict(type='POD', U=g['U'], q_ref=g['q_ref'], v_ref=g['v_ref'])
    src, dst = str(tmp_path / 'tpwl.pkl'), str(tmp_path / 'lin.pkl')
    save_data(src, tpwl)
    TPWL2LinearROM(src, dst)
    lin = load_data(dst)
    assert sorted(lin.keys()) == list(g['lin_keys'])
    for k in ('A_c', 'B_c', 'd_c'):
        np.testing.assert_array_equal(lin[k], g['lin_' + k])
        np.testing.assert_array_equal(lin[k], g['model_' + k][0])
    np.testing.assert_array_equal(lin['rom_info']['U'], g['lin_rom_U'])
    assert lin['rom_info']['type'] == str(g['lin_rom_type'])


def test_header_declares_the_new_entry_points():
    src = open(os.path.join(ROOT, 'include', 'sofacontrol_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name in ('sric_dare_wide', 'srompc_create', 'srompc_destroy', 'srompc_set_gains', 'srompc_set_state', 'srompc_get_state',
                 'srompc_initialize', 'srompc_step', 'srompc_replay', 'srompc_stats'):
        assert re.search(r'^\s*int\s+%s\s*\(' % name, src, flags=re.M), name
    assert 'typedef struct srompc srompc_t;' in src
