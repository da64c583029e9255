"""Linear reduced-order model of the ROMPC baseline -- surface of sofacontrol/baselines/rompc/rompc_utils.py:7-147.

`LinearROM` is one continuous-time affine model (A_c, B_c, d_c) in POD coordinates, discretised once by the device
zero-order hold (`utils.zoh_affine`, csrc/discretize.hip).  Measurement / output maps are the full-order selectors pushed
through the basis: C = Cf V, y_ref = Cf x_ref (and H, z_ref likewise), so "y" below means the offset-free reduced
measurement and "yf" the full-order one.

Two defects of the reference are not kept (behavioural notes): `x_to_zy(y=True)` multiplies C by the flag
instead of the state (rompc_utils.py:111), and `get_rom_info` reads an attribute that is never set (:128)."""
import numpy as np

from ... import utils as scutils
from ...mor import pod


class LinearROM:
    def __init__(self, data, dt, Cf=None, Hf=None):
        model = data if isinstance(data, dict) else scutils.load_data(data)
        self._rom_info = model['rom_info']
        if self._rom_info['type'] != 'POD':
            raise NotImplementedError("Unknown ROM type")
        self.A_d, self.B_d, self.d_d = scutils.zoh_affine(model['A_c'], model['B_c'], model['d_c'], dt)
        self.rom = pod.POD(self._rom_info)
        self.state_dim = self.N = self.A_d.shape[0]
        self.input_dim = self.B_d.shape[1]
        self.C = self.y_ref = self.meas_dim = None
        self.H = self.z_ref = self.output_dim = None
        if Cf is not None:
            self.set_measurement_model(Cf)
        if Hf is not None:
            self.set_output_model(Hf)

    # -- dynamics ------------------------------------------------------------------------------------------------
    def get_jacobians(self, x, dt):
        """The model is the same everywhere: (A_d, B_d, d_d) whatever x and dt are (rompc_utils.py:44-45)."""
        return self.A_d, self.B_d, self.d_d

    @staticmethod
    def update_dynamics(x, u, A_d, B_d, d_d):
        return A_d @ x + np.squeeze(B_d @ u) + d_d

    def update_state(self, x, u):
        return LinearROM.update_dynamics(x, u, self.A_d, self.B_d, self.d_d)

    # -- maps ----------------------------------------------------------------------------------------------------
    def _reduce(self, Mf):
        M = Mf @ self.rom.V
        return np.asarray(M, dtype=np.float64), np.asarray(Mf @ self.rom.x_ref, dtype=np.float64).ravel()

    def set_measurement_model(self, Cf):
        self.C, self.y_ref = self._reduce(Cf)
        self.meas_dim = self.C.shape[0]

    def set_output_model(self, Hf):
        self.H, self.z_ref = self._reduce(Hf)
        self.output_dim = self.H.shape[0]

    def _offset(self, zv, yv, sign):
        """Add (sign = +1) or remove (-1) the reference offset of whichever quantity was passed, outputs first."""
        if zv is not None and self.z_ref is not None:
            return zv + sign * self.z_ref
        if yv is not None and self.y_ref is not None:
            return yv + sign * self.y_ref
        raise RuntimeError('Need to set output or meas. model')

    def zfyf_to_zy(self, zf=None, yf=None):
        return self._offset(zf, yf, -1.0)

    def zy_to_zfyf(self, z=None, y=None):
        return self._offset(z, y, +1.0)

    def _map(self, x, want_z, want_y):
        """(matrix, offset) applied to rows of x: the output model when asked for and present, else the measurement model."""
        if want_z and self.H is not None:
            return np.transpose(self.H @ x.T), self.z_ref
        if want_y and self.C is not None:
            return np.transpose(self.C @ x.T), self.y_ref
        raise RuntimeError('Need to set output or meas. model')

    def x_to_zfyf(self, x, zf=False, yf=False):
        v, ref = self._map(x, zf, yf)
        return v + ref

    def x_to_zy(self, x, z=False, y=False):
        return self._map(x, z, y)[0]

    # -- sizes ---------------------------------------------------------------------------------------------------
    def get_state_dim(self):
        return self.state_dim

    def get_input_dim(self):
        return self.input_dim

    def get_output_dim(self):
        return self.output_dim

    def get_meas_dim(self):
        return self.meas_dim

    def get_rom_info(self):
        return self._rom_info


def TPWL2LinearROM(tpwl_loc, save_loc):
    """A linear model file out of a TPWL model file: its first linearisation point and its basis (rompc_utils.py:131-147).
    Host I/O only."""
    tpwl = scutils.load_data(tpwl_loc)
    linear = {k: tpwl[k][0] for k in ('A_c', 'B_c', 'd_c')}
    linear['rom_info'] = tpwl['rom_info']
    scutils.save_data(save_loc, linear)
