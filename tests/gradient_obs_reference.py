"""Host restatement of the observation's part of ``aog_output_gradient`` on the separable route (``aog_upload_gradient_obs``,
include/aogym.h) in numpy float64, written from the header's definition and not from the library's route through W and H.

Per env, with phi the sensing-arm phase of tests/gradient_reference.py on the packed aperture pixels p = (y_p, x_p) and E_p = exp(i phi_p):

    F_vu = sum_p m1[v, y_p] E_p m2[x_p, u],   obs_raw[v o + u] = |F_vu|^2   (m1 = tables.obs_m1 [o, N], m2 = tables.obs_m2 [N, o])

The gradient is J' gbar with the dense Jacobian of every |F_vu|^2 with respect to every pixel's phase,
J[vu, p] = 2 Re(conj(F_vu) i E_p m1[v, y_p] m2[x_p, u]), then through d phi_p / d a_k = (4 pi / lambda_wfs) M_pk; the power and Strehl rows are
those of gradient_reference.  Cotangents and values are [.., o^2 + 2]: the observation, power, Strehl."""
import numpy as np

import gradient_reference as gr


def _kernels(tables):
    """A1 [o, n_ap] = m1[v, y_p], A2 [n_ap, o] = m2[x_p, u]."""
    m1, m2 = np.asarray(tables.obs_m1, dtype=np.complex128), np.asarray(tables.obs_m2, dtype=np.complex128)
    N = m1.shape[1]
    ap = np.asarray(tables.ap_index)
    return m1[:, ap // N], m2[ap % N, :]


def field(phi, tables):
    """F [B, o, o] for phases phi [B, n_ap]."""
    A1, A2 = _kernels(tables)
    return np.stack([(A1 * np.exp(1j * p)[None, :]) @ A2 for p in phi])


def values_of(phi, tables):
    """[B, o^2 + 2]: obs_raw, power, strehl."""
    F = field(phi, tables)
    return np.concatenate([(np.abs(F) ** 2).reshape(len(phi), -1), gr.values_of(phi, tables)], axis=1)


def jacobian_phi(phi_e, tables):
    """Dense Jacobian [o^2 + 2, n_ap] of one env's values with respect to its pixels' phases."""
    A1, A2 = _kernels(tables)
    E = np.exp(1j * phi_e)
    F = (A1 * E[None, :]) @ A2
    o = F.shape[0]
    dF = 1j * E[None, None, :] * A1[:, None, :] * A2.T[None, :, :]   # [v, u, p]
    J = 2.0 * np.real(np.conj(F)[:, :, None] * dF).reshape(o * o, -1)
    return np.concatenate([J, gr.jacobian_phi(phi_e, tables)], axis=0)


def grad_actuators(screens, actuators, tables, gbar):
    """dL/d actuators for cotangents gbar [B, o^2 + 2] -> [B, A], or a stack [K, B, o^2 + 2] -> [K, B, A] (one Jacobian per env for all K)."""
    g = np.asarray(gbar, dtype=np.float64)
    many = g.ndim == 3
    g = g if many else g[None]
    phi = gr.phase(screens, actuators, tables)
    dphi = 4.0 * np.pi / float(tables.params.wavelength_wfs) * np.asarray(tables.modes, dtype=np.float64)   # [n_ap, A]
    out = np.empty((g.shape[0], len(phi), dphi.shape[1]))
    for e in range(len(phi)):
        out[:, e] = (g[:, e] @ jacobian_phi(phi[e], tables)) @ dphi
    return out if many else out[0]
