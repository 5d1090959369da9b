"""Host restatement of ``aog_output_gradient`` (include/aogym.h) in numpy float64, written from the header's definition and independent of
the library's route through C and H.

Per env, phi_p = 2 pi w_p / lambda_wfs is the sensing-arm phase on packed aperture pixel p (w: the optical path error of
tests/wavefront_reference.py, from the screens, the actuators and the mode matrix), E = exp(i phi), E_sci = exp(i r phi) with
r = lambda_wfs / lambda_sci, and with the pupil-plane kernels K = coef @ tables

    Z = K_wfs E,  obs_raw = |Z_j|^2 (the rows before the fiber modes),  power = sum |Z_k|^2 (the fiber-mode rows),  strehl = |K_sci E_sci|^2.

The gradient is formed as J' gbar with the dense Jacobian of every value with respect to every pixel's phase,
J[j, p] = 2 Re(conj(Z_j) i E_p K[j, p]), then through d phi_p / d a_k = (4 pi / lambda_wfs) M_pk.  The action chain (AO_env.py:119-120) is
differentiated explicitly: the dense Jacobian of a = c v / sqrt(v' G v) with respect to v, v_k = action_k / (k + 10)."""
import numpy as np

import wavefront_reference as wr


def _lams(tables):
    return float(tables.params.wavelength_wfs), float(tables.params.wavelength_sci)


def phase(screens, actuators, tables):
    """phi [B, n_ap] radians at the sensing wavelength."""
    return 2.0 * np.pi * wr.path_error(screens, actuators, tables) / _lams(tables)[0]


def _kernels(tables):
    Kw = np.asarray(tables.wfs_coef, dtype=np.complex128) @ np.asarray(tables.wfs_tables, dtype=np.float64)   # [n_out, n_ap]
    Ks = np.asarray(tables.sci_coef, dtype=np.complex128).reshape(1, -1) @ np.asarray(tables.sci_tables, dtype=np.float64)   # [1, n_ap]
    return Kw, Ks


def values_of(phi, tables):
    """[B, n_obs + 2]: obs_raw, power, strehl (n_obs = 0 on the separable route's tables)."""
    lw, ls = _lams(tables)
    Kw, Ks = _kernels(tables)
    n_obs = Kw.shape[0] - tables.n_fiber_modes
    Z = np.exp(1j * phi) @ Kw.T
    Zs = np.exp(1j * (lw / ls) * phi) @ Ks.T
    pw = np.abs(Z) ** 2
    return np.concatenate([pw[:, :n_obs], pw[:, n_obs:].sum(axis=1, keepdims=True), np.abs(Zs) ** 2], axis=1)


def jacobian_phi(phi_e, tables):
    """Dense Jacobian [n_obs + 2, n_ap] of one env's values with respect to its pixels' phases."""
    lw, ls = _lams(tables)
    r = lw / ls
    Kw, Ks = _kernels(tables)
    n_obs = Kw.shape[0] - tables.n_fiber_modes
    E, Es = np.exp(1j * phi_e), np.exp(1j * r * phi_e)
    Z, Zs = Kw @ E, Ks @ Es
    Jw = 2.0 * np.real(np.conj(Z)[:, None] * (1j * E[None, :] * Kw))
    Js = 2.0 * r * np.real(np.conj(Zs)[:, None] * (1j * Es[None, :] * Ks))
    return np.concatenate([Jw[:n_obs], Jw[n_obs:].sum(axis=0, keepdims=True), Js], axis=0)


def cotangent(g_obs, g_power, g_strehl, B, n_obs):
    """[B, n_obs + 2] from the three cotangents (None = zero)."""
    g = np.zeros((B, n_obs + 2))
    if g_obs is not None and n_obs:
        g[:, :n_obs] = g_obs
    if g_power is not None:
        g[:, n_obs] = g_power
    if g_strehl is not None:
        g[:, n_obs + 1] = g_strehl
    return g


def grad_actuators(screens, actuators, tables, gbar):
    """dL/d actuators [B, A] for cotangents gbar [B, n_obs + 2] (per metre of surface)."""
    phi = phase(screens, actuators, tables)
    dphi = 4.0 * np.pi / _lams(tables)[0] * np.asarray(tables.modes, dtype=np.float64)   # [n_ap, A]
    return np.stack([(gbar[e] @ jacobian_phi(phi[e], tables)) @ dphi for e in range(len(phi))])


def actuators_of_action(action, tables):
    """AO_env.py:119-120: v = action / (k + 10), a = c v / sqrt(v' G v)."""
    a = np.asarray(action, dtype=np.float64)
    v = a / (np.arange(a.shape[1]) + 10.0)
    G = np.asarray(tables.gram, dtype=np.float64)
    n = np.sqrt(np.einsum("ei,ij,ej->e", v, G, v))
    c = tables.params.action_rms_fraction * _lams(tables)[1]
    return c * v / n[:, None]


def chain_to_action(grad_act, action, tables):
    """dL/d action from dL/d actuators through the dense Jacobian of the normalisation."""
    a = np.asarray(action, dtype=np.float64)
    k10 = np.arange(a.shape[1]) + 10.0
    G = np.asarray(tables.gram, dtype=np.float64)
    c = tables.params.action_rms_fraction * _lams(tables)[1]
    out = np.empty_like(a)
    for e in range(len(a)):
        v = a[e] / k10
        Gv = G @ v
        n = np.sqrt(v @ Gv)
        Jav = c * (np.eye(len(v)) / n - np.outer(v, Gv) / n ** 3)   # d a_i / d v_j
        out[e] = (grad_act[e] @ Jav) / k10
    return out


def host_state(env):
    """(screens, actuators) of a ``BatchedAOEnv`` in its current state, as numpy."""
    return env.get_screens().cpu().numpy(), env.get_actuators().cpu().numpy()
