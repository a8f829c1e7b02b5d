"""The steady-state criterion of MembraneModel.steady_state / knpemi_ode_advance, restated on the host."""
import numpy as np


def steady_steps(traj, rtol, atol, window):
    """traj[k, q, j]: state j of node q after k steps (k = 0: the start).  After step k a node is still when every
    component moved by at most atol + rtol |y(k)|; it is steady after `window` still steps in a row, and the function
    returns that k per node (-1: never)."""
    traj = np.asarray(traj, np.float64)
    still = (np.abs(traj[1:] - traj[:-1]) <= atol + rtol * np.abs(traj[1:])).all(axis=2)
    out = np.full(traj.shape[1], -1, np.int64)
    run = np.zeros(traj.shape[1], np.int64)
    for k in range(still.shape[0]):
        run = np.where(still[k], run + 1, 0)
        newly = (out < 0) & (run >= window)
        out[newly] = k + 1
    return out
