"""Host restatement of include/aogym_conjugate.h in numpy float64, written from the header's text: the altitude mirror's surface (products
and sums in mode order, each rounded on its own), the fit of a layer's logical screen, and the installation with mirrors — the sightline
restatement (tests/sightline_reference.py) with the surfaces appended to the layers' screens.  numpy's float64 ``*`` and ``+`` are single
correctly rounded operations and nothing here is fused, so the device's surfaces and a float64 front's ``psi64`` must match bit for bit."""
import numpy as np

import sightline_reference as sref


def surface(cmd, basis):
    """[B, M M]: s = cmd[b][0] basis[0][p]; s = s + (cmd[b][k] basis[k][p]) for k = 1 .. K - 1.  ``cmd`` [B, K], ``basis`` [K, M M]."""
    cmd, basis = np.asarray(cmd, dtype=np.float64), np.asarray(basis, dtype=np.float64)
    basis = basis.reshape(basis.shape[0], -1)
    s = cmd[:, 0:1] * basis[0][None, :]
    for k in range(1, basis.shape[0]):
        s = s + (cmd[:, k:k + 1] * basis[k][None, :])
    return s


def set_command(old_cmd, old_surface, cmd, basis, mask=None):
    """(command, surface) after aog_altmirror_set_command: the selected envs take ``cmd`` and its surface, the others keep theirs."""
    sel = np.ones(len(cmd), dtype=bool) if mask is None else np.asarray(mask) != 0
    command, surf = np.array(old_cmd, dtype=np.float64), np.array(old_surface, dtype=np.float64)
    command[sel] = np.asarray(cmd, dtype=np.float64)[sel]
    surf[sel] = surface(cmd, basis)[sel]
    return command, surf


def fit(fit_rows, screens):
    """(value [B, K], bound [B, K]): sum_p fit[k][p] screen_b[p] over the logical screens [B, M, M], and the header's bound on any fixed
    order of that sum, M M 2^-53 sum_p |fit[k][p] screen_b[p]|."""
    f = np.asarray(fit_rows, dtype=np.float64)
    s = np.asarray(screens, dtype=np.float64).reshape(len(screens), -1)
    terms = s[:, None, :] * f[None, :, :]
    return terms.sum(axis=2), s.shape[1] * 2.0 ** -53 * np.abs(terms).sum(axis=2)


def install(screens, surfaces, shifts, ap_index, N, wavelength_wfs, coeff=None, basis=None):
    """What aog_install_layer_sum_conjugate leaves in a front: ``sightline_reference.install`` with the mirrors' surfaces ([B, M_j, M_j]
    each) as further sources behind the layers' screens; ``shifts`` [L + n_mirrors, B, 2]."""
    sources = list(screens) + [np.asarray(s, dtype=np.float64) for s in surfaces]
    assert len(sources) == len(shifts) <= 8
    return sref.install(sources, shifts, ap_index, N, wavelength_wfs, coeff, basis)
