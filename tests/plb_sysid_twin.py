"""NumPy restatement of the identification loop's optimiser side (PlasticineLab sim2sim / real2sim plb/optimizer/optim.py:52-72 Adam with
the learning rates (lr, lr / 50000, lr), and solver.py:70-74: pin, clip, floor), per env row, and of the chamfer distance
(solver.py:187-196) in the operation order include/unidom_hip.h states.  The specification unidom_amd/algorithms/plb_identify.py and
ud_plb_chamfer are held to (tests/test_plb_sysid_cpu.py, tests/test_plb_sysid_gpu.py)."""
import numpy as np


class AdamTwin:
    def __init__(self, parameters, lr=100.0, beta_1=0.9, beta_2=0.999, epsilon=1e-8):
        self.parameters = np.array(parameters, np.float64)          # [B,3], the optimiser's own: never clipped
        self.lr = np.array([lr, lr / 50000, lr])
        self.beta_1, self.beta_2, self.epsilon = beta_1, beta_2, epsilon
        self.m = np.zeros_like(self.parameters)
        self.v = np.zeros_like(self.parameters)
        self.iter = 0

    def step(self, grads):
        gd = np.asarray(grads, np.float64).reshape(self.parameters.shape)
        self.m = self.beta_1 * self.m + (1 - self.beta_1) * gd
        self.v = self.beta_2 * self.v + (1 - self.beta_2) * (gd * gd)
        m_cap = self.m / (1 - self.beta_1 ** (self.iter + 1))
        v_cap = self.v / (1 - self.beta_2 ** (self.iter + 1))
        self.iter += 1
        self.parameters = self.parameters - (self.lr * m_cap) / (np.sqrt(v_cap) + self.epsilon)
        return self.parameters.copy()


def constrain(parameters, pin=(None, None, 200.0), bounds=((None, None), (0.2, 0.4), (None, None))):
    p = np.array(parameters, np.float64)
    for k, value in enumerate(pin):
        if value is not None:
            p[:, k] = value
    for k, (lo, hi) in enumerate(bounds):
        if lo is not None or hi is not None:
            p[:, k] = np.clip(p[:, k], lo, hi)
    return np.clip(p, 0.01, 9999999999999999)


def chamfer(a, b):
    """a [Na,3], b [Nb,3] -> (out, min_ab [Na], min_ba [Nb]); d = sqrt((dx dx + dy dy) + dz dz)."""
    d = a[:, None, :] - b[None, :, :]
    dist = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    mab, mba = np.min(dist, axis=1), np.min(dist, axis=0)
    return np.mean(mab) + np.mean(mba), mab, mba
