"""Host restatement of the gradient of the modulated pyramid sensor's frames and slopes with respect to the mirror's actuators (DESIGN.md §5,
"Pyramid sensor: gradient"; include/aogym.h, aog_pyramid_gradient), float64 numpy, on top of pyramid_reference.Sensor.

Two statements that share no intermediate: the dense Jacobians (forward mode: one perturbed field per actuator) and the vector-Jacobian
product ``grad`` (reverse mode: the W, V, H, q chain the device runs).  The CPU tests hold the first to finite differences of ``Sensor``'s
own frames and slopes and the second to the first.

u = psi + 2 M a / lambda_wfs in revolutions, E = exp(2 pi i u) on the aperture, F_j = m1_j E m2_j, G_{q,j} = b_{sy} F_j b_{sx}' over the
quadrant's own block, I_q = (1 / n_mod) sum_j |G_{q,j}|^2, q = 2 sy + sx."""
import numpy as np

import pyramid_reference as ref


def _halves(sensor):
    wq = sensor.wq
    return (slice(0, wq), slice(wq, 2 * wq))


def _sides(sensor, j):
    """(L [2][n_s, N], R [2][N, n_s]) of modulation point j: G_{q,j} = L[sy] E R[sx]."""
    hv = _halves(sensor)
    L = [sensor.b[:, h] @ sensor.m1[j][h, :] for h in hv]
    R = [sensor.m2[j][:, h] @ sensor.b[:, h].T for h in hv]
    return L, R


def frame_jacobian(sensor, modes, wavelength_wfs, u_rev):
    """d frame / d actuators: [4, n_s, n_s, A] (per metre of surface, the units of get_actuators())."""
    N, ns, A = sensor.N, sensor.ns, modes.shape[1]
    E = sensor.field(u_rev)
    # dE / da_k = 2 pi i E (2 / lambda) M_k on the aperture
    dE = np.zeros((A, N * N), dtype=np.complex128)
    dE[:, sensor.ap_index] = (2j * np.pi * E.ravel()[sensor.ap_index])[None, :] * (2.0 / wavelength_wfs) * np.asarray(modes, dtype=np.float64).T
    dE = dE.reshape(A, N, N)
    J = np.zeros((4, ns, ns, A))
    for j in range(sensor.n_mod):
        L, R = _sides(sensor, j)
        for sy in range(2):
            for sx in range(2):
                G = L[sy] @ E @ R[sx]
                dG = np.einsum("ay,kyx,xb->kab", L[sy], dE, R[sx])
                J[2 * sy + sx] += 2.0 * np.moveaxis((np.conj(G)[None] * dG).real, 0, -1)
    return J / sensor.n_mod


def slopes_jacobian_of_frame(sensor, frame):
    """d slopes / d frame: [2 n_valid, 4, n_s^2], the dependence on the mean quadrant sum included."""
    ns, nv = sensor.ns, sensor.valid.size
    I = np.asarray(frame, dtype=np.float64).reshape(4, -1)[:, sensor.valid]
    ibar = I.sum(axis=0).mean()
    s = sensor.slopes_of(frame)
    D = np.zeros((2 * nv, 4, ns * ns))
    sign = np.array([[-1.0, 1.0, -1.0, 1.0], [-1.0, -1.0, 1.0, 1.0]])      # s_x, s_y over the quadrants
    for axis in range(2):
        for k in range(nv):
            D[axis * nv + k, :, sensor.valid[k]] += sign[axis] / ibar
        # - s / Ibar x d Ibar, d Ibar = (1 / n_valid) sum over valid pixels and quadrants
        D[axis * nv:(axis + 1) * nv][:, :, sensor.valid] -= (s[axis * nv:(axis + 1) * nv] / (ibar * nv))[:, None, None]
    return D


def jacobians(sensor, modes, wavelength_wfs, u_rev):
    """(d frame / da [4, n_s, n_s, A], d slopes / da [2 n_valid, A])."""
    Jf = frame_jacobian(sensor, modes, wavelength_wfs, u_rev)
    D = slopes_jacobian_of_frame(sensor, sensor.frame(u_rev))
    return Jf, D.reshape(D.shape[0], -1) @ Jf.reshape(-1, Jf.shape[-1])


def slopes_cotangent_to_frame(sensor, frame, g_slopes):
    """The cotangent on the frame [4, n_s, n_s] that a cotangent on the slopes [2 n_valid] pulls back to."""
    ns, nv = sensor.ns, sensor.valid.size
    I = np.asarray(frame, dtype=np.float64).reshape(4, -1)[:, sensor.valid]
    ibar = I.sum(axis=0).mean()
    s = sensor.slopes_of(frame)
    g = np.asarray(g_slopes, dtype=np.float64)
    gx, gy = g[:nv], g[nv:]
    c = float(g @ s) / (nv * ibar)
    out = np.zeros((4, ns * ns))
    out[0, sensor.valid] = (-gx - gy) / ibar - c
    out[1, sensor.valid] = (gx - gy) / ibar - c
    out[2, sensor.valid] = (-gx + gy) / ibar - c
    out[3, sensor.valid] = (gx + gy) / ibar - c
    return out.reshape(4, ns, ns)


def grad(sensor, screen, modes, actuators, wavelength_wfs, g_frames=None, g_slopes=None):
    """dL / d actuators [A] of L = sum(g_frames * frame) + sum(g_slopes * slopes) at (screen, actuators), by the reverse chain:
    W = gbar conj(G) / n_mod, V = the window with block q = b_{sy}' W_q b_{sx}, H = m1_j' V m2_j', q_p = sum_j 2 Re(2 pi i E_p H_p),
    dL/da_k = (2 / lambda_wfs) sum_p M_pk q_p.  Also returns the clean frame and slopes: (grad, frame, slopes)."""
    assert g_frames is not None or g_slopes is not None
    modes = np.asarray(modes, dtype=np.float64)
    u = ref.phase_rev(screen, modes, actuators, sensor.ap_index, wavelength_wfs)
    E = sensor.field(u)
    frame = sensor.frame(u)
    gbar = np.zeros((4, sensor.ns, sensor.ns))
    if g_frames is not None:
        gbar = gbar + np.asarray(g_frames, dtype=np.float64).reshape(gbar.shape)
    if g_slopes is not None:
        gbar = gbar + slopes_cotangent_to_frame(sensor, frame, g_slopes)
    hv = _halves(sensor)
    w = 2 * sensor.wq
    q = np.zeros(sensor.N * sensor.N)
    for j in range(sensor.n_mod):
        F = sensor.focal(E, j)
        V = np.zeros((w, w), dtype=np.complex128)
        for sy in range(2):
            for sx in range(2):
                G = sensor.b[:, hv[sy]] @ F[hv[sy], hv[sx]] @ sensor.b[:, hv[sx]].T
                W = gbar[2 * sy + sx] * np.conj(G) / sensor.n_mod
                V[hv[sy], hv[sx]] = sensor.b[:, hv[sy]].T @ W @ sensor.b[:, hv[sx]]
        H = sensor.m1[j].T @ V @ sensor.m2[j].T
        q += (2.0 * (2j * np.pi * E * H).real).ravel()
    g = (2.0 / wavelength_wfs) * (modes.T @ q[sensor.ap_index])
    return g, frame, sensor.slopes_of(frame)
