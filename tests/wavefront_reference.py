"""Host restatement of ``aog_wavefront_truth`` (include/aogym.h), independent of the library's route through the normal equations.

Per env the optical path error over the n aperture pixels is ``w = s / (2 pi) + 2 M a`` (s: the achromatic screen on the aperture, M: the
mode matrix, a: the actuators).  The best correction the mirror can make is the least-squares fit of w on ``[1, M]`` (a free piston and the
modes), solved here by ``numpy.linalg.lstsq`` (SVD of the design matrix itself):

    rms      std of w over the aperture
    fit_rms  RMS of that fit's residual (unique, whatever the rank of [1, M])
    coef     the modes' coefficients.  Where [1, M] has full column rank they are the lstsq solution's.  A piston mode (Zernike 1) makes
             [1, M] rank-deficient and the split of the constant term between the intercept and that mode arbitrary; the definition gives a
             mode without variance over the aperture the coefficient 0, which is the minimum-norm solution of the CENTRED system
             ``lstsq(M - column means, w)`` — so that is what is solved for the coefficients in every case (the same fit: the tests check
             that both systems leave the same residual).
    ideal_actuators  a - coef / 2 (path = 2 x surface)
"""
import numpy as np


def path_error(screens, actuators, tables):
    """w [B, n_ap] float64 from full-grid screens [B, N, N] (hcipy's unit, phase x lambda), actuators [B, A] (metres) and the host tables."""
    s = np.asarray(screens, dtype=np.float64).reshape(len(screens), -1)[:, np.asarray(tables.ap_index)]
    return s / (2.0 * np.pi) + 2.0 * np.asarray(actuators, dtype=np.float64) @ np.asarray(tables.modes, dtype=np.float64).T


def truth_of(w, modes, actuators):
    """The four results for path errors w [B, n_ap]."""
    modes = np.asarray(modes, dtype=np.float64)
    B, n = w.shape
    A = modes.shape[1]
    X = np.concatenate([np.ones((n, 1)), modes], axis=1)
    Mc = modes - modes.mean(axis=0)
    out = dict(rms=np.empty(B), fit_rms=np.empty(B), coef=np.empty((B, A)), ideal_actuators=np.empty((B, A)))
    for e in range(B):
        sol = np.linalg.lstsq(X, w[e], rcond=None)[0]
        res = w[e] - X @ sol
        coef = np.linalg.lstsq(Mc, w[e], rcond=None)[0]
        res_c = (w[e] - w[e].mean()) - Mc @ coef
        assert abs(np.sqrt(np.mean(res_c ** 2)) - np.sqrt(np.mean(res ** 2))) <= 1e-12 * w[e].std(), "the two least-squares systems disagree"
        out["rms"][e] = w[e].std()
        out["fit_rms"][e] = np.sqrt(np.mean(res ** 2))
        out["coef"][e] = coef
        out["ideal_actuators"][e] = np.asarray(actuators[e], dtype=np.float64) - coef / 2.0
    return out


def host_truth(env):
    """The restatement for a ``BatchedAOEnv`` in its current state: phase from ``get_screens()``, ``get_actuators()`` and ``env.tables.modes``."""
    act = env.get_actuators().cpu().numpy()
    return truth_of(path_error(env.get_screens().cpu().numpy(), act, env.tables), env.tables.modes, act)
