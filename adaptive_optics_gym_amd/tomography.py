"""A tomographic controller: the classical baseline of the altitude mirrors (multi-conjugate AO).

``LayeredAOEnv(altitude_mirrors=...)`` puts correctors at altitude, and every sightline reads its own footprint of them.  The question
they raise — which commands of the pupil mirror and the altitude mirrors TOGETHER leave the least residual over a set of directions — is
linear least squares: along guide direction g the residual path error is ``w_g = (atmosphere)_g + T_g' x``, x the stacked unknowns (the
pupil mirror's A actuators, then every altitude mirror's K_m commands) and ``T_g`` [K_tot, n_ap] their response on that front
(``sightline_shapes``).  With ``b_g = T_g (w_g - mean)`` the minimiser of ``sum_g w_g |w_g|^2`` moves x by ``- H^-1 sum_g w_g b_g``,
``H = sum_g w_g T_g T_g'`` (``reconstructor``).  ``TomographicController.fit()`` is that one-shot ceiling, read from the true residual
wavefronts (``aog_wavefront_project``: the footprints do not lie in the span of the pupil modes, which is all ``wavefront_truth`` projects
onto); ``action()`` is the loop that reaches it, an integrator on the device (``aog_tomo_update``) fed by a measurement on every guide
front.  Device side: ``include/aogym_tomography.h``, ``csrc/k_tomography.h``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .device_handle import DeviceHandle, ptr

MEASUREMENTS = ("truth", "modal")
COND_LIMIT = 1e12


# ---- host geometry (float64 numpy) ---------------------------------------------------------------------------------------------------------
def _one_shift(shift, j):
    """(sx, sy) of mirror j from [2] or per-env [B, 2] values, which must agree across the batch."""
    s = np.asarray(shift, dtype=np.float64)
    if s.ndim == 2:
        if not np.all(s == s[0]):
            raise ValueError(f"sightline_shapes: the shift of mirror {j} differs across the batch (per-env angles): this version takes one "
                             "geometry for the whole batch")
        s = s[0]
    if s.shape != (2,) or not np.all(np.isfinite(s)):
        raise ValueError(f"sightline_shapes: the shift of mirror {j} must be a finite (sx, sy) pair, got shape {s.shape}")
    return float(s[0]), float(s[1])


def _one_magnification(m, j):
    """m of mirror j from a scalar or per-env [B] values, which must agree across the batch; None stays None (a plane wave)."""
    if m is None:
        return None
    m = np.asarray(m, dtype=np.float64).reshape(-1)
    if not np.all(m == m[0]):
        raise ValueError(f"sightline_shapes: the magnification of mirror {j} differs across the batch (per-env ranges): this version takes one "
                         "geometry for the whole batch")
    if not 0.0 < m[0] <= 1.0:
        raise ValueError(f"sightline_shapes: the magnification of mirror {j} must lie in (0, 1], got {m[0]!r}")
    return float(m[0])


def displaced_basis(basis, shift, ap_index, N, magnification=None):
    """[K, n_ap]: the [K, M, M] ``basis`` read bilinearly at (iy + c + sy, ix + c + sx), c = (M - N) / 2, on the aperture pixels
    (iy, ix) = divmod(ap_index, N) — the read of the installation (include/aogym_sightline.h), value for value:
    ``(gy ((gx v00) + (fx v01))) + (fy ((gx v10) + (fx v11)))``, indices modulo M.  With a ``magnification`` m (a source at finite range:
    include/aogym_cone.h) the read is that header's instead, at (c + ctr + m (iy - ctr) + sy, c + ctr + m (ix - ctr) + sx), ctr = (N - 1) / 2,
    per axis ``s0 = floor(s); q = ((m - 1) (i - ctr)) + (s - s0); q0 = floor(q); f = q - q0; g = 1 - f``, first index ``i + s0 + q0`` — at
    m = 1 the sightline read to the bit."""
    b = np.asarray(basis, dtype=np.float64)
    M = b.shape[-1]
    if b.ndim != 3 or b.shape[1] != M or M < N or (M - N) % 2:
        raise ValueError(f"sightline_shapes: a basis must be [K, M, M] with M >= {N} and M - {N} even, got shape {b.shape}")
    c = (M - N) // 2
    sx, sy = shift
    iy, ix = np.divmod(np.asarray(ap_index, dtype=np.int64), N)
    if magnification is None:
        x0, y0 = np.floor(sx), np.floor(sy)
        fx, fy = sx - x0, sy - y0
        gx, gy = 1.0 - fx, 1.0 - fy
        py, px = (iy + c + int(y0)) % M, (ix + c + int(x0)) % M
    else:
        k, ctr = float(magnification) - 1.0, 0.5 * (N - 1)
        sx0, sy0 = np.floor(sx), np.floor(sy)
        qy, qx = (k * (iy - ctr)) + (sy - sy0), (k * (ix - ctr)) + (sx - sx0)
        y0, x0 = np.floor(qy), np.floor(qx)
        fx, fy = qx - x0, qy - y0
        gx, gy = 1.0 - fx, 1.0 - fy
        py, px = (iy + c + int(sy0) + y0.astype(np.int64)) % M, (ix + c + int(sx0) + x0.astype(np.int64)) % M
    py1, px1 = (py + 1) % M, (px + 1) % M
    top = (gx * b[:, py, px]) + (fx * b[:, py, px1])
    bottom = (gx * b[:, py1, px]) + (fx * b[:, py1, px1])
    return (gy * top) + (fy * bottom)


def sightline_shapes(env_or_tables, mirrors, shifts_g, pupil_mirror=True, num_pupil_pixels=None, magnifications=None):
    """T_g [K_tot, n_ap] float64: the path error in metres on the aperture pixels of one front per unit of each unknown — the pupil
    mirror's A actuators first (``2 x modes``: path = 2 x surface, ``ideal_actuators = actuators - coef / 2``; left out with
    ``pupil_mirror=False``), then every altitude mirror's K_m commands, its basis read at that front's shift and cropped to the pupil as
    the installation reads it, converted from the master screens' unit to metres (/ 2 pi).

    env_or_tables  an env (``tables``, ``num_pupil_pixels``) or its host tables (then ``num_pupil_pixels`` is given)
    mirrors        objects with ``basis`` [K_m, M, M] (``conjugate.AltitudeMirror``), or such arrays
    shifts_g       [n_mirrors, 2] (sx, sy) in pixels of this front, or [n_mirrors, B, 2] whose envs agree (``ValueError`` otherwise)
    magnifications None (a plane-wave front), or per mirror the magnification of its footprint on this front ([n_mirrors] or
                   [n_mirrors, B] whose envs agree): the mirror is then read as ``aog_install_layer_sum_cone`` reads it"""
    tables = getattr(env_or_tables, "tables", env_or_tables)
    N = int(num_pupil_pixels if num_pupil_pixels is not None else env_or_tables.num_pupil_pixels)
    shifts_g = np.asarray(shifts_g, dtype=np.float64)
    if len(shifts_g) != len(mirrors):
        raise ValueError(f"sightline_shapes: {len(mirrors)} mirrors, {len(shifts_g)} shifts")
    rows = [2.0 * np.asarray(tables.modes, dtype=np.float64).T] if pupil_mirror else []
    if magnifications is not None and len(magnifications) != len(mirrors):
        raise ValueError(f"sightline_shapes: {len(mirrors)} mirrors, {len(magnifications)} magnifications")
    for j, m in enumerate(mirrors):
        mag = None if magnifications is None else _one_magnification(magnifications[j], j)
        rows.append(displaced_basis(getattr(m, "basis", m), _one_shift(shifts_g[j], j), tables.ap_index, N, mag) / (2.0 * np.pi))
    if not rows:
        raise ValueError("sightline_shapes: no unknowns (no altitude mirror and pupil_mirror=False)")
    return np.ascontiguousarray(np.concatenate(rows, axis=0))


def centred(T):
    """The rows of T with their aperture means removed."""
    T = np.asarray(T, dtype=np.float64)
    return T - T.mean(axis=1, keepdims=True)


def tilt_projected(T, ap_index, N):
    """T P [K, n_ap], P = I - t t' over the aperture's tip and tilt: t [n_ap, 2] the x and y coordinates of the aperture pixels, centred
    and orthonormalised.  What a guide star that cannot see tip and tilt (a laser: the upward and downward paths cancel them) contributes:
    every row of the result has zero inner product with any tilt of the front, so ``T P w`` does not move when a tilt is added to w."""
    T = np.asarray(T, dtype=np.float64)
    iy, ix = np.divmod(np.asarray(ap_index, dtype=np.int64), N)
    t = np.stack([ix - ix.mean(), iy - iy.mean()], axis=1).astype(np.float64)
    t, _ = np.linalg.qr(t)
    return T - (T @ t) @ t.T


def _regularised_inverse(H, alpha, who):
    K = H.shape[0]
    H = 0.5 * (H + H.T)
    # an unknown no guide front answers to at all (the pupil mirror's piston: its centred response is zero) stays at zero: its row and
    # column of the inverse are zeros, and it counts neither in the trace's mean nor in the condition number
    seen = np.flatnonzero(np.diag(H) > 1e-24 * np.diag(H).max())
    Hs = H[np.ix_(seen, seen)]
    Hs = Hs + (float(alpha) * np.trace(Hs) / len(seen)) * np.eye(len(seen))
    cond = np.linalg.cond(Hs)
    if not np.isfinite(cond) or cond > COND_LIMIT:
        raise ValueError(f"{who}: the normal matrix has condition number {cond:.3g} > {COND_LIMIT:g} at alpha = {alpha:g}: the guide directions "
                         "do not determine every unknown (raise alpha, add a guide star, or drop unknowns)")
    inv = np.zeros((K, K))
    inv[np.ix_(seen, seen)] = np.linalg.pinv(Hs, hermitian=True)
    return 0.5 * (inv + inv.T)


def normal_matrix(T_list, weights):
    """H = sum_g w_g Tc_g Tc_g' [K_tot, K_tot], Tc_g the row-centred T_g."""
    H = None
    for T, w in zip(T_list, weights):
        Tc = centred(T)
        H = w * (Tc @ Tc.T) if H is None else H + w * (Tc @ Tc.T)
    return H


def reconstructor(T_list, weights, alpha):
    """H^-1 [K_tot, K_tot], symmetric: ``H = sum_g w_g Tc_g Tc_g' + alpha tr(H) / K_tot I``.  ``ValueError`` naming the condition number
    when it exceeds 1e12 (with alpha = 0: unknowns the guide directions cannot tell apart).  One exception to the formula: an unknown
    whose centred response is zero on every guide front (diagonal of H below 1e-24 of the largest: the pupil mirror's piston) gets zero
    rows and columns and counts neither in tr(H) / K_tot nor in the condition number — it can be neither seen nor used."""
    weights = _weights(weights, len(T_list))
    return _regularised_inverse(normal_matrix(T_list, weights), alpha, "reconstructor")


def modal_interaction(T, modes, fit):
    """D [A, K_tot]: what ``wavefront_truth()["coef"]`` of a front answers per unit of each unknown, ``fit (Mc' T')``."""
    Mc = centred(np.asarray(modes, dtype=np.float64).T)
    return np.asarray(fit, dtype=np.float64) @ (Mc @ centred(T).T)


def modal_reconstructors(D_list, weights, alpha):
    """R_g [K_tot, A] per guide front: the blocks of the regularised least-squares inverse of the stacked modal interaction matrix,
    ``R_g = w_g (sum_g w_g D_g' D_g + alpha tr / K_tot I)^-1 D_g'``."""
    weights = _weights(weights, len(D_list))
    H = None
    for D, w in zip(D_list, weights):
        H = w * (D.T @ D) if H is None else H + w * (D.T @ D)
    inv = _regularised_inverse(H, alpha, "modal_reconstructors")
    return [np.ascontiguousarray(w * (inv @ D.T)) for D, w in zip(D_list, weights)]


def _weights(weights, G):
    w = np.ones(G) if weights is None else np.asarray(weights, dtype=np.float64)
    if w.shape != (G,) or not np.all(np.isfinite(w)) or np.any(w <= 0):
        raise ValueError(f"weights: one positive finite weight per guide star ({G}), got {weights!r}")
    return w


# ---- the bare handle -------------------------------------------------------------------------------------------------------------------------
class DeviceTomograph(DeviceHandle):
    """The library handle (``aog_tomo``) alone: per env a command u [n_out] float64 and the update
    ``u <- clip(leak u - gain sum_g R_g s_g, +-stroke)`` from ``len(widths)`` inputs s_g [batch, widths[g]] (``update``); ``upload(g, R)``
    sets R_g [n_out, widths[g]].  Every product and sum is rounded on its own in the order g, then j (``tests/tomography_reference.py``
    replays it bit for bit).  The state blob of ``get_state`` / ``set_state`` is u [batch, n_out] float64."""

    prefix, noun = "aog_tomo", "tomograph"

    def __init__(self, batch, n_out, widths, env_id_base=0, device=None):
        import torch

        self.batch, self.n_out, self.widths, self.env_id_base = int(batch), int(n_out), tuple(int(w) for w in widths), int(env_id_base)
        if self.batch < 1:
            raise ValueError(f"DeviceTomograph: num_envs must be >= 1, got {batch!r}")
        if not 1 <= self.n_out <= _lib.TOMO_MAX_OUT:
            raise ValueError(f"DeviceTomograph: n_out must lie in 1 .. {_lib.TOMO_MAX_OUT}, got {n_out!r}")
        if not 1 <= len(self.widths) <= _lib.TOMO_MAX_INPUTS:
            raise ValueError(f"DeviceTomograph: n_inputs must lie in 1 .. {_lib.TOMO_MAX_INPUTS}, got {len(self.widths)} widths")
        for g, w in enumerate(self.widths):
            if not 1 <= w <= _lib.TOMO_MAX_WIDTH:
                raise ValueError(f"DeviceTomograph: width[{g}] must lie in 1 .. {_lib.TOMO_MAX_WIDTH}, got {w}")
        if self.env_id_base < 0:
            raise ValueError(f"DeviceTomograph: env_id_base must be >= 0, got {env_id_base!r}")
        self._bind(torch, device, self.batch)
        self._create()

    def _config(self):
        width = (C.c_int32 * 4)(*(self.widths + (0,) * (4 - len(self.widths))))
        return _lib.AogTomoConfig(_lib.ABI_VERSION, self.batch, self.n_out, len(self.widths), width, self.env_id_base, 0)

    def upload(self, g, R):
        """R_g [n_out, widths[g]] (anything ``torch.as_tensor`` takes) becomes input g's matrix."""
        torch = self._torch
        if not 0 <= int(g) < len(self.widths):
            raise ValueError(f"upload: g must lie in 0 .. {len(self.widths) - 1}, got {g!r}")
        r = torch.as_tensor(R, device=self.device).to(torch.float64).contiguous()
        if tuple(r.shape) != (self.n_out, self.widths[g]):
            raise ValueError(f"upload: R must be [{self.n_out}, {self.widths[g]}], got {list(r.shape)}")
        self._call("upload", int(g), ptr(r), self._stream())
        torch.cuda.current_stream(self.device).synchronize()   # (r may be a temporary)

    def update(self, inputs, gain, leak=1.0, stroke=0.0, mask=None, out=None):
        """One update of the selected envs; returns u [batch, n_out] of every env as it stands after the call (``out``: a tensor to write)."""
        torch = self._torch
        if len(inputs) != len(self.widths):
            raise ValueError(f"update: {len(self.widths)} inputs expected, got {len(inputs)}")
        rows = [self._tensor(s, (self.batch, w), torch.float64, f"update: inputs[{g}] must be a contiguous float64 [{self.batch}, {w}] tensor on {self.device}")
                for g, (s, w) in enumerate(zip(inputs, self.widths))]
        m = self._mask(mask, "update")
        shape = (self.batch, self.n_out)
        out = torch.empty(shape, dtype=torch.float64, device=self.device) if out is None else self._tensor(
            out, shape, torch.float64, f"update: out must be a contiguous float64 {list(shape)} tensor on {self.device}")
        ptrs = (C.c_void_p * len(rows))(*[r.data_ptr() for r in rows])
        self._call("update", ptrs, float(gain), float(leak), float(stroke), ptr(m), ptr(out), self._stream())
        return out

    def reset(self, mask=None):
        self._call("reset", ptr(self._mask(mask, "reset")), self._stream())

    command = property(lambda self: self.get_state().view(self._torch.float64).reshape(self.batch, self.n_out), doc="[batch, n_out] float64: u as it stands")


# ---- the projection on a front ---------------------------------------------------------------------------------------------------------------
def upload_wavefront_shapes(front, shapes):
    """``shapes`` [K, n_ap] float64 become the shapes ``wavefront_project(front)`` projects onto (``aog_upload_wavefront_shapes``)."""
    s = np.ascontiguousarray(shapes, dtype=np.float64)
    if s.ndim != 2 or s.shape[1] != int(front.tables.n_ap):
        raise ValueError(f"upload_wavefront_shapes: shapes must be [K, {int(front.tables.n_ap)}], got {s.shape}")
    _lib.check(front.lib.aog_upload_wavefront_shapes(front._handle, s.ctypes.data_as(C.c_void_p), int(s.shape[0])))
    front._wavefront_shapes = int(s.shape[0])


def wavefront_project(front, out=None, mean=None):
    """[B, K] float64: ``sum_p S[k][p] (w_bp - mean_b)`` of the front's residual path error in metres at its current state
    (``aog_wavefront_project``); ``mean`` ([B] float64 tensor, optional) receives the aperture means.  Stream-ordered, no host
    synchronisation, nothing a step reads is changed.  ``RuntimeError`` (``_lib.AogError``) before ``upload_wavefront_shapes`` and while a
    pipelined or policy-attached step has an action pending, like ``wavefront_truth``."""
    torch = front._torch
    K = getattr(front, "_wavefront_shapes", None)
    if K is None:
        raise _lib.AogError("wavefront_project: no shapes were uploaded (upload_wavefront_shapes)")
    B = int(front.num_envs)

    def held(t, shape, name):   # the library writes B K (or B) float64 values at the address it is given
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or not t.is_contiguous() or tuple(t.shape) != shape
                or t.device != torch.empty(0, device=front.device).device):
            raise ValueError(f"wavefront_project: {name} must be a contiguous float64 {list(shape)} tensor on {front.device}")

    if out is None:
        out = torch.empty((B, K), dtype=torch.float64, device=front.device)
    else:
        held(out, (B, K), "out")
    if mean is not None:
        held(mean, (B,), "mean")
    _lib.check(front.lib.aog_wavefront_project(front._handle, ptr(out), ptr(mean), front._stream()))
    return out


# ---- the controller --------------------------------------------------------------------------------------------------------------------------
class TomographicController:
    """The tomographic (MCAO) controller of a ``LayeredAOEnv`` built with ``altitude_mirrors`` and without ``altitude_action``.

    guide_stars   the directions the residual is minimised over: ``"self"`` (the env's own front) and names of its sightlines.
    weights       one positive weight per guide star (default 1 each).
    measurement   what is measured on every guide front:
                  ``"truth"``   ``aog_wavefront_project`` onto the centred T_g: ``s_g = b_g`` [B, K_tot], ``R_g = w_g H^-1`` — the loop
                                whose fixed point is ``fit()``;
                  ``"modal"``   ``wavefront_truth()["coef"]`` [B, A]: a perfect sensor limited to the pupil mirror's modes;
                                ``R_g`` = ``modal_reconstructors``' block.
    gain, leak, stroke   ``u <- clip(leak u - gain sum_g R_g s_g, +-stroke)`` (``stroke <= 0``: no clip); alpha: the regularisation of H.
    pupil_mirror  False: only the altitude mirrors are unknowns; ``action()`` then returns the pupil mirror's actuators as they stand.
    tilt_blind    names of guide stars that do not see tip and tilt (a laser guide star: the upward and downward paths cancel them).  The
                  shapes uploaded for ``aog_wavefront_project`` on such a front and its rows of the normal matrix are ``T_g P``
                  (``tilt_projected``): whatever tip and tilt its wavefront carries moves neither ``action()`` nor ``fit()``.  Host side
                  only, and for ``measurement="truth"`` only: a ``"modal"`` measurement is the front's modal coefficients, tilt included,
                  which the projected rows do not take out again (``ValueError``).  With every guide star blind nothing determines the
                  unknowns' tip and tilt, and construction raises.

    A guide front that looks at a source at finite range (``LayeredAOEnv(source_range=)``, ``add_sightline(range=)``) gets its ``T_g`` from the
    cone read of the mirrors (``sightline_shapes(magnifications=)``), value for value what ``aog_install_layer_sum_cone`` installs.

    ``action(out=None)`` measures on every guide front, runs one ``aog_tomo_update``, sets every altitude mirror's command to its slice of u
    and returns the pupil mirror's [B, A] float64 actuators in ``ideal_action()``'s form (the action of an env built with
    ``SH_operation=True``); ``update(measurements)`` does the same from the caller's measurements.  The integrator assumes the mirrors
    hold its u: ``reset(mask)`` it with the env when episodes start flat.  ``fit()`` is the one-shot ceiling — the least-squares u* over
    the guide directions at the current state, ``u - H^-1 sum_g w_g b_g`` from the true residuals — and writes no state.
    ``state_dict()`` / ``load_state_dict()`` resume bit-identically; everything runs on the caller's current stream.  One geometry for the
    whole batch: per-env angles that differ raise ``ValueError``.

    The geometry is read at construction: after ``set_field_angle`` / ``Sightline.set_angle`` on a guide direction ``action()`` and
    ``fit()`` raise ``ValueError`` (build a new controller); with ``from_parts`` the shifts are the caller's to keep.

    ``from_parts(fronts, mirrors, shifts, ...)`` builds it on stand-alone pieces instead: static fronts (``BatchedAOEnv``) that get their
    screens from ``conjugate.install_layer_sum_conjugate``, ``AltitudeMirror`` objects and, per front, the mirrors' shifts [n_mirrors, 2];
    the caller installs, and hands the returned actuators to its fronts."""

    def __init__(self, env, guide_stars=("self",), weights=None, measurement="truth", gain=0.5, leak=1.0, alpha=1e-6, stroke=0.0, pupil_mirror=True,
                 tilt_blind=()):
        mirrors = list(getattr(env, "altitude_mirrors", None) or ())
        if not mirrors:
            raise ValueError("TomographicController: the env has no altitude mirrors (LayeredAOEnv(altitude_mirrors=[...])); without them "
                             "policy='ideal' is the controller")
        if getattr(env, "_altitude_scale", None) is not None:
            raise ValueError("TomographicController: the env was built with altitude_action, which hands the altitude mirrors to the action; "
                             "build it without")
        guide_stars = (guide_stars,) if isinstance(guide_stars, str) else tuple(guide_stars)
        fronts, shifts, mags = [], [], []
        n_layers = len(env.layers)
        for name in guide_stars:
            if name == "self" or name in env.sightlines:
                holder = env if name == "self" else env.sightlines[name]
                fronts.append(env if name == "self" else holder.env), shifts.append(holder._shifts[n_layers:])
                # (a front at finite range is installed through its cone geometry: T_g restates that read)
                geometry = getattr(holder, "_geometry", None)
                mags.append(None if geometry is None else geometry[n_layers:, :, 2])
            else:
                raise ValueError(f"TomographicController: unknown guide star {name!r} (\"self\" or one of the env's sightlines {sorted(env.sightlines)})")
        self.env = env
        self._build(fronts, mirrors, shifts, guide_stars, weights, measurement, gain, leak, alpha, stroke, pupil_mirror, mags, tilt_blind)
        # the geometry is read once: T_g, H^-1 and the uploaded shapes belong to these shifts (_check_geometry)
        self._looked = [(env if name == "self" else env.sightlines[name], np.array(s, copy=True)) for name, s in zip(guide_stars, shifts)]

    @classmethod
    def from_parts(cls, fronts, mirrors, shifts, weights=None, measurement="truth", gain=0.5, leak=1.0, alpha=1e-6, stroke=0.0, pupil_mirror=True,
                   magnifications=None, tilt_blind=()):
        self = cls.__new__(cls)
        self.env = None
        if not mirrors:
            raise ValueError("TomographicController: no altitude mirrors")
        self._build(list(fronts), list(mirrors), list(shifts), tuple(f"front{g}" for g in range(len(fronts))), weights, measurement, gain, leak,
                    alpha, stroke, pupil_mirror, magnifications, tilt_blind)
        return self

    def _build(self, fronts, mirrors, shifts, names, weights, measurement, gain, leak, alpha, stroke, pupil_mirror, magnifications=None, tilt_blind=()):
        if measurement not in MEASUREMENTS:
            raise ValueError(f"measurement must be 'truth' or 'modal' (got {measurement!r})")
        if not 1 <= len(fronts) <= _lib.TOMO_MAX_INPUTS:
            raise ValueError(f"TomographicController: 1 .. {_lib.TOMO_MAX_INPUTS} guide stars, got {len(fronts)}")
        if len(set(names)) != len(names):
            raise ValueError(f"TomographicController: a guide star is named twice in {names!r}")
        for v, what in ((gain, "gain"), (leak, "leak"), (alpha, "alpha"), (stroke, "stroke")):
            if not np.isfinite(float(v)):
                raise ValueError(f"TomographicController: {what} must be finite, got {v!r}")
        if float(alpha) < 0:
            raise ValueError(f"TomographicController: alpha must be >= 0, got {alpha!r}")
        self.guide_stars, self.measurement, self.pupil_mirror = tuple(names), measurement, bool(pupil_mirror)
        self.gain, self.leak, self.alpha, self.stroke = float(gain), float(leak), float(alpha), float(stroke)
        self.weights = _weights(weights, len(fronts))
        self.fronts, self.mirrors = fronts, mirrors
        first = fronts[0]
        self.num_envs, self.num_modes, self.device = int(first.num_envs), int(first.num_modes), first.device
        # the geometry, on the host
        tilt_blind = (tilt_blind,) if isinstance(tilt_blind, str) else tuple(tilt_blind)
        for name in tilt_blind:
            if name not in names:
                raise ValueError(f"TomographicController: tilt_blind names {name!r}, which is no guide star of {names!r}")
        if tilt_blind and measurement != "truth":
            raise ValueError("TomographicController: tilt_blind needs measurement='truth' (a 'modal' measurement carries the front's tip and tilt "
                             "in its coefficients, which the projected shapes do not remove)")
        self.tilt_blind = tilt_blind
        magnifications = [None] * len(fronts) if magnifications is None else list(magnifications)
        if len(magnifications) != len(fronts):
            raise ValueError(f"TomographicController: {len(fronts)} guide stars, {len(magnifications)} sets of magnifications")
        self.T = [sightline_shapes(first, mirrors, s, self.pupil_mirror, magnifications=m) for s, m in zip(shifts, magnifications)]
        self.T = [tilt_projected(T, first.tables.ap_index, int(first.num_pupil_pixels)) if name in tilt_blind else T for T, name in zip(self.T, names)]
        self.n_unknowns = int(self.T[0].shape[0])
        if self.n_unknowns > _lib.WAVEFRONT_MAX_SHAPES:
            raise ValueError(f"TomographicController: {self.n_unknowns} unknowns, aog_wavefront_project takes {_lib.WAVEFRONT_MAX_SHAPES} shapes")
        self.slices = []   # of u, per altitude mirror
        lo = self.num_modes if self.pupil_mirror else 0
        for m in mirrors:
            self.slices.append(slice(lo, lo + int(m.n_modes)))
            lo += int(m.n_modes)
        try:
            self.H_inv = reconstructor(self.T, self.weights, self.alpha)
        except ValueError as err:
            if set(names) <= set(tilt_blind):
                raise ValueError(f"{err}.  Every guide star is in tilt_blind: no front measures tip and tilt, so the unknowns' own tip and tilt are "
                                 "undetermined — add a guide star that sees them (a natural star: leave it out of tilt_blind)") from None
            raise
        R_truth = [np.ascontiguousarray(w * self.H_inv) for w in self.weights]
        if measurement == "truth":
            self.R = R_truth
        else:
            from .optics_host import wavefront_fit

            modes = np.asarray(first.tables.modes, dtype=np.float64)
            fit = wavefront_fit(modes)
            self.R = modal_reconstructors([modal_interaction(T, modes, fit) for T in self.T], self.weights, self.alpha)
        # the device side: the centred T_g as every guide front's shapes (fit() reads them whatever the measurement), the integrator, and a
        # second handle for fit(), which must write no state of the loop's
        for front, T in zip(fronts, self.T):
            upload_wavefront_shapes(front, centred(T))
        base = int(getattr(first, "global_env_offset", 0))
        self.tomo = DeviceTomograph(self.num_envs, self.n_unknowns, [R.shape[1] for R in self.R], base, self.device)
        for g, R in enumerate(self.R):
            self.tomo.upload(g, R)
        self._ceiling = DeviceTomograph(self.num_envs, self.n_unknowns, [self.n_unknowns] * len(fronts), base, self.device)
        for g, R in enumerate(R_truth):
            self._ceiling.upload(g, R)

    def _check_geometry(self, who):
        """``ValueError`` when a guide direction of the env has moved since construction (``set_field_angle``, ``Sightline.set_angle``,
        ``set_state`` with other angles): T_g, H^-1 and the shapes on the fronts are those of the old geometry — build a new controller."""
        n_layers = len(self.env.layers) if self.env is not None else 0
        for name, (holder, then) in zip(self.guide_stars, getattr(self, "_looked", ())):
            if not np.array_equal(holder._shifts[n_layers:], then):
                raise ValueError(f"TomographicController.{who}: guide star {name!r} looks along another angle than the controller was built for; its "
                                 "reconstructor is that of the old geometry — build a new TomographicController")

    # -- measurements --
    def _measure(self, g):
        front = self.fronts[g]
        if getattr(front, "_next_actions_keepalive", None) is not None:
            raise ValueError("TomographicController.action: a pipelined step has an action pending (the mirror already belongs to the next step)")
        if self.measurement == "truth":
            return wavefront_project(front)
        return front.wavefront_truth()["coef"]

    def _apply(self, u, out):
        for m, sl in zip(self.mirrors, self.slices):
            m.set_command(u[:, sl].contiguous())
        a = u[:, :self.num_modes] if self.pupil_mirror else self.fronts[0].get_actuators()
        if out is None:
            return a.contiguous()
        out.copy_(a)
        return out

    def action(self, out=None):
        self._check_geometry("action")
        return self.update([self._measure(g) for g in range(len(self.fronts))], out=out)

    def update(self, measurements, mask=None, out=None):
        u = self.tomo.update(list(measurements), self.gain, self.leak, self.stroke, mask)
        return self._apply(u, out)

    @property
    def command(self):
        """u [B, K_tot] float64 as the integrator holds it."""
        return self.tomo.command

    def mirror_state(self):
        """[B, K_tot] float64: the unknowns as the mirrors hold them now — the first guide front's actuators, then the altitude mirrors' commands."""
        torch = self.fronts[0]._torch
        parts = ([self.fronts[0].get_actuators()] if self.pupil_mirror else []) + [m.command for m in self.mirrors]
        return torch.cat(parts, dim=1).contiguous()

    def normal_residual(self):
        """[B, K_tot] float64: ``sum_g w_g b_g`` at the current state, zero at the least-squares optimum."""
        total = None
        for w, front in zip(self.weights, self.fronts):
            b = wavefront_project(front) * float(w)
            total = b if total is None else total + b
        return total

    def fit(self):
        """u* [B, K_tot] float64: the least-squares unknowns over the guide directions at the current state, ``u - H^-1 sum_g w_g b_g`` with u
        what the mirrors hold and b_g the projections of the true residuals.  Writes no state of the loop or the mirrors."""
        self._check_geometry("fit")
        torch = self.fronts[0]._torch
        u = self.mirror_state()
        self._ceiling.set_state(u.view(torch.uint8).reshape(-1))
        return self._ceiling.update([wavefront_project(f) for f in self.fronts], 1.0, 1.0, 0.0)

    def reset(self, mask=None):
        self.tomo.reset(mask)

    def state_dict(self):
        return {"blob": self.tomo.get_state(), "n_unknowns": self.n_unknowns, "batch": self.num_envs, "measurement": self.measurement,
                "guide_stars": self.guide_stars}

    def load_state_dict(self, state):
        for k, have in (("n_unknowns", self.n_unknowns), ("batch", self.num_envs), ("measurement", self.measurement), ("guide_stars", self.guide_stars)):
            if tuple(state[k]) != tuple(have) if isinstance(have, tuple) else state[k] != have:
                raise ValueError(f"load_state_dict: the state was taken with {k} = {state[k]!r}, this controller has {have!r}")
        self.tomo.set_state(state["blob"])

    def close(self):
        self.tomo.close()
        self._ceiling.close()
