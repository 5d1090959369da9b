"""``LayeredAOEnv`` — a multi-layer frozen-flow atmosphere: several wind layers per env.

A single frozen-flow screen is a pure translation; a site has a slow ground layer and fast high layers moving in other directions, and
their sum is what makes a one-frame control lag cost Strehl.  On axis and conjugated to the pupil, L layers are exactly the sum of L
independent screens, so every layer here is an ordinary dynamic ``BatchedAOEnv`` that only evolves (``evolve_atmosphere``), one kernel
sums the layers' float64 master screens into the screen tiles of a quasi-static FRONT handle (``install_layer_sum``), and the front
steps with the static fused kernel it already has.  Everything that reads the front's screens — reset, step, the separable observation
route, Shack-Hartmann, ``wavefront_truth``, the science camera, ``output_gradient``, ``step_with_policy``, ``step_with_spgd``, pipelined steps — works on it
unchanged.

With ``layer_altitudes`` the layers leave the pupil plane: a layer at altitude h is seen displaced by h x angle along a line of sight at
that angle, so it is drawn on a meta-pupil larger than the pupil and every front — the env's own (``field_angle``) and any number of
further ``Sightline`` fronts over the same layers (``add_sightline``) — reads it at its own sub-pixel shift
(``aog_install_layer_sum_sightline``).  The part of the wavefront that differs between two sightlines is angular anisoplanatism: no
controller that senses on one of them removes it on the other.  ``altitude_mirrors`` adds the corrector that acts on it: deformable
mirrors conjugated to altitudes (``conjugate.AltitudeMirror``), whose surfaces every front reads displaced like a layer at that altitude.
"""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from .batched_env import BatchedAOEnv, _mask_array
from .params import resolve_per_env, resolve_turbulence

MAX_LAYERS = 8   # aog_install_layer_sum's limit


def layer_seed(seed, layer):
    """The seed of layer ``layer``'s own env — the one place it is derived.  Layer 0 takes the env's ``seed`` unchanged (a one-layer env
    draws what a plain dynamic env with that seed draws); layer l > 0 takes the first 31-bit word of
    ``numpy.random.SeedSequence([base, l])``, base = ``seed`` (1234 when None, as ``BatchedAOEnv``): a hash, so that it collides neither
    with another layer's nor with the ``seed + global env id`` streams of the envs."""
    if layer == 0:
        return seed
    base = 1234 if seed is None else int(seed)
    return int(np.random.SeedSequence([base & 0xFFFFFFFFFFFFFFFF, int(layer)]).generate_state(1)[0] & 0x7FFFFFFF)


def resolve_layers(atm_layers, atm_fried, num_envs, total_envs=None, global_env_offset=0):
    """``atm_layers`` checked and split: a list of dict(fraction, fried, speed) — what layer l's env is built with.  ``atm_layers``:
    1 .. 8 of ``{"fraction": f_l, "speed": v_l}``; the fractions of the turbulence strength are positive and sum to 1 within 1e-12, each
    speed is a scalar or per-env values under ``atm_vel``'s rules.  Layer l runs at r0_l = r0 f_l^(-3/5) (per env when ``atm_fried`` is),
    so that the layers' Cn^2 add up to the Cn^2 of the requested r0 (Cn^2 is proportional to r0^(-5/3)).  ``ValueError`` for anything
    else, before anything is created."""
    total_envs = global_env_offset + num_envs if total_envs is None else int(total_envs)
    if atm_layers is None or isinstance(atm_layers, dict) or not 1 <= len(atm_layers) <= MAX_LAYERS:
        raise ValueError(f"atm_layers: expected a list of 1 .. {MAX_LAYERS} dicts {{'fraction': f, 'speed': v}}")
    fractions = []
    for lay in atm_layers:
        if not isinstance(lay, dict) or set(lay) != {"fraction", "speed"}:
            raise ValueError("atm_layers: every layer is a dict with exactly the keys 'fraction' and 'speed'")
        f = float(lay["fraction"])
        if not np.isfinite(f) or f <= 0:
            raise ValueError(f"atm_layers: fractions must be positive and finite, got {lay['fraction']!r}")
        fractions.append(f)
    if abs(float(np.sum(fractions)) - 1.0) > 1e-12:
        raise ValueError(f"atm_layers: the fractions must sum to 1 within 1e-12, got {float(np.sum(fractions))!r}")
    resolve_turbulence("dynamic", atm_fried, 1, num_envs, total_envs, global_env_offset, False)   # (the total r0's own checks)
    fried = np.asarray(atm_fried, dtype=np.float64)
    out = []
    for f, lay in zip(fractions, atm_layers):
        fried_l = fried * f ** (-3.0 / 5.0)
        fried_l = float(fried_l) if fried_l.ndim == 0 else fried_l
        resolve_turbulence("dynamic", fried_l, lay["speed"], num_envs, total_envs, global_env_offset, False)
        out.append(dict(fraction=f, fried=fried_l, speed=lay["speed"]))
    return out


def resolve_altitudes(layer_altitudes, num_layers):
    """``layer_altitudes`` checked: [L] float64 metres, one per layer, finite and >= 0 (None stays None: every layer in the pupil plane).
    ``ValueError`` otherwise."""
    if layer_altitudes is None:
        return None
    h = np.asarray(layer_altitudes, dtype=np.float64)
    if h.ndim != 1 or h.size != num_layers:
        raise ValueError(f"layer_altitudes: expected one altitude in metres per layer ({num_layers}), got shape {h.shape}")
    if not np.all(np.isfinite(h)) or np.any(h < 0):
        raise ValueError("layer_altitudes: altitudes must be finite and >= 0")
    return h.copy()


def resolve_field_angle(angle, num_envs, total_envs=None, global_env_offset=0, name="field_angle"):
    """A line of sight as [num_envs, 2] float64 radians (theta_x, theta_y): one pair for every env, or per-env pairs [num_envs, 2] /
    [total_envs, 2] under ``resolve_per_env``'s rules (the latter indexed by global env id).  None is on axis.  ``ValueError`` otherwise."""
    total_envs = global_env_offset + num_envs if total_envs is None else int(total_envs)
    if angle is None:
        return np.zeros((num_envs, 2))
    a = np.asarray(angle, dtype=np.float64)
    if a.shape == (2,):
        cols = (a[0], a[1])
    elif a.ndim == 2 and a.shape[1] == 2:
        cols = (a[:, 0], a[:, 1])
    else:
        raise ValueError(f"{name}: expected (theta_x, theta_y) in radians or an array [num_envs, 2] / [total_envs, 2], got shape {a.shape}")
    return np.stack([resolve_per_env(name, c, num_envs, total_envs, global_env_offset)[0] for c in cols], axis=1)


def sightline_shifts(altitudes, angle, pupil_pixel):
    """[L, B, 2] float64 (sx, sy) in pixels: layer l at altitude h_l is read h_l theta / pupil_pixel further along +x / +y by a front that
    looks along theta = (theta_x, theta_y) — front pixel (iy, ix) reads the layer's meta-pupil at (iy + c + sy, ix + c + sx).  One rounded
    product and one rounded quotient per value, in that order."""
    h = np.asarray(altitudes, dtype=np.float64)
    a = np.asarray(angle, dtype=np.float64)
    return np.ascontiguousarray((h[:, None, None] * a[None, :, :]) / float(pupil_pixel))


def required_margin(altitudes, angles, pupil_pixel, guard=0):
    """The margin c (pixels on every side) a meta-pupil needs for the sightlines ``angles`` (a list of [B, 2] arrays):
    ceil(max |h_l theta| / pupil_pixel) + 1 — the integer part of the shift and the bilinear read's second sample — plus ``guard``, the
    band a ``scintillation`` keeps between every footprint and the meta-pupil's edge (``scintillation.default_guard``)."""
    worst = 0.0
    for a in angles:
        s = sightline_shifts(altitudes, a, pupil_pixel)
        worst = max(worst, float(np.abs(s).max()) if s.size else 0.0)
    return int(np.ceil(worst)) + 1 + int(guard)


def default_meta_pupil_pixels(num_pupil_pixels, margin):
    """The smallest meta-pupil N_L >= N + 2 margin the dynamic handle accepts as a layer of a front with N pixels: N_L - N even (the
    meta-pupil is centred on the pupil) and, for N a multiple of 4, N_L a multiple of 4 as well (the two-band screen synthesis and the
    ring's vector rows are built for such sizes)."""
    n = int(num_pupil_pixels) + 2 * int(margin)
    if num_pupil_pixels % 4 == 0:
        n = (n + 3) // 4 * 4
    return n


def check_margin(shifts, margins, what, first_mirror=None):
    """``ValueError`` unless every shift of layer l lies inside its margin: |s| <= c_l - 1, exactly 0 for c_l = 0 (what the library checks
    again).  ``shifts`` [L, B, 2], ``margins`` [L].  ``first_mirror``: sources from that index on are altitude mirrors, named "mirror j"."""
    for l, c in enumerate(margins):
        limit = max(int(c) - 1, 0)
        worst = float(np.abs(shifts[l]).max())
        if not np.isfinite(worst) or worst > limit:
            source = f"layer {l}" if first_mirror is None or l < first_mirror else f"mirror {l - first_mirror}"
            raise ValueError(f"{what}: {source} would be read {worst:.3f} pixels off the pupil, its meta-pupil leaves {limit} "
                             f"(margin c = {int(c)}; build the env with a larger meta_pupil_pixels)")


def resolve_range(value, num_envs, total_envs=None, global_env_offset=0, name="source_range"):
    """A source's range as [num_envs] float64 metres: None or inf is a plane wave (inf for every env), otherwise a scalar or per-env values
    under ``resolve_per_env``'s rules, each > 0 and not NaN (inf is allowed per env).  ``ValueError`` otherwise."""
    total_envs = global_env_offset + num_envs if total_envs is None else int(total_envs)
    if value is None:
        return np.full(num_envs, np.inf)
    arr = np.asarray(value, dtype=np.float64)
    if np.any(np.isnan(arr)) or np.any(arr <= 0):
        raise ValueError(f"{name}: a range is in metres, > 0 (inf or None: a plane wave), got {value!r}")
    # (resolve_per_env refuses inf: it is this argument's 'none', so it goes through as a finite stand-in)
    far = np.isinf(arr)
    out = resolve_per_env(name, np.where(far, 1.0, arr), num_envs, total_envs, global_env_offset)[0]
    mask = resolve_per_env(name, far.astype(np.float64), num_envs, total_envs, global_env_offset)[0]
    return np.where(mask != 0, np.inf, out)


def _source_name(l, first_mirror):
    return f"layer {l}" if first_mirror is None or l < first_mirror else f"mirror {l - first_mirror}"


def cone_geometry(altitudes, angle, range, pupil_pixel, first_mirror=None, what="source_range"):
    """[S, B, 3] float64 (sx, sy, m): ``sightline_shifts`` and, beside them, the magnification of source l's footprint seen from a source at
    ``range`` ([B] metres, or a scalar; inf: a plane wave), m = 1 - h_l / H — one rounded quotient and one rounded difference, so m is
    exactly 1.0 for H = inf and for h_l = 0.  Front pixel (iy, ix) reads the source at (c + ctr + m (iy - ctr) + sy, c + ctr + m (ix - ctr)
    + sx), ctr = (N - 1) / 2 (include/aogym_cone.h).  ``ValueError`` naming the layer (or mirror, from index ``first_mirror`` on) that lies at
    or above the source (h_l >= H)."""
    h = np.asarray(altitudes, dtype=np.float64)
    shifts = sightline_shifts(h, angle, pupil_pixel)
    H = np.broadcast_to(np.asarray(range, dtype=np.float64), (shifts.shape[1],))
    if np.any(np.isnan(H)) or np.any(H <= 0):
        raise ValueError(f"{what}: a range is in metres, > 0 (inf: a plane wave)")
    for l, b in np.argwhere(h[:, None] >= H[None, :]):
        raise ValueError(f"{what}: {_source_name(int(l), first_mirror)} at {h[l]:g} m lies at or above the source at {H[b]:g} m (env {int(b)}): a "
                         "layer or mirror must be below every source that is seen through it")
    m = 1.0 - (h[:, None] / H[None, :])
    return np.ascontiguousarray(np.concatenate([shifts, m[:, :, None]], axis=2))


def cone_reach(geometry, num_pupil_pixels):
    """[S] float64: how far off the pupil source l is read, max over envs and axes of |s| + (1 - m) (N - 1) / 2 — the shift plus what the
    shrinking footprint's far edge adds on the side the shift points away from (one rounded difference, product and sum, as the library)."""
    g = np.asarray(geometry, dtype=np.float64)
    ctr = 0.5 * (int(num_pupil_pixels) - 1)
    return (np.abs(g[:, :, :2]) + ((1.0 - g[:, :, 2:3]) * ctr)).reshape(len(g), -1).max(axis=1)


def declared_range(value):
    """A range argument as the 1-D array of every value it declares, whichever envs this instance holds (None: [inf]): what the default
    meta-pupil is sized for, so that the parts of a split batch and the whole batch get one size."""
    return np.array([np.inf]) if value is None else np.atleast_1d(np.asarray(value, dtype=np.float64)).ravel()


def required_margin_cone(altitudes, looks, pupil_pixel, num_pupil_pixels):
    """``required_margin`` for sources at finite range: ``looks`` a list of (angle [B, 2], ranges), ranges a 1-D array of any length (the
    local envs', or every declared value: ``declared_range``).  Per source l the largest |h_l theta| / pupil_pixel over the angles plus the
    largest (1 - m) (N - 1) / 2 over the ranges — a shrinking footprint moves its far edge that many pixels off the plane wave's — then
    ceil(max_l) + 1.  The two maxima are taken apart, so the result does not depend on which env has which range; with every range
    infinite it is ``required_margin``.  ``ValueError`` when a source lies at or above one of the ranges."""
    h = np.asarray(altitudes, dtype=np.float64)
    ctr = 0.5 * (int(num_pupil_pixels) - 1)
    worst = 0.0
    for a, H in looks:
        H = np.atleast_1d(np.asarray(H, dtype=np.float64))
        m = cone_geometry(h, np.zeros((H.size, 2)), H, pupil_pixel)[:, :, 2]
        s = np.abs(sightline_shifts(h, a, pupil_pixel)).reshape(len(h), -1)
        if s.size:
            worst = max(worst, float((s.max(axis=1) + ((1.0 - m) * ctr).max(axis=1)).max()))
    return int(np.ceil(worst)) + 1


def check_margin_cone(geometry, margins, num_pupil_pixels, what, first_mirror=None):
    """``check_margin`` for sources at finite range: ``ValueError`` unless |s| + (1 - m) (N - 1) / 2 <= c_l - 1 for every source (0 for
    c_l = 0: no shift and m = 1), and 0 < m <= 1 — what the library checks again.  ``geometry`` [S, B, 3], ``margins`` [S]."""
    g = np.asarray(geometry, dtype=np.float64)
    m = g[:, :, 2]
    if not np.all(np.isfinite(g)) or np.any(m <= 0) or np.any(m > 1):
        raise ValueError(f"{what}: shifts must be finite and magnifications lie in (0, 1]")
    reach = cone_reach(g, num_pupil_pixels)
    for l, c in enumerate(margins):
        limit = max(int(c) - 1, 0)
        if reach[l] > limit:
            raise ValueError(f"{what}: {_source_name(l, first_mirror)} would be read {reach[l]:.3f} pixels off the pupil (shift plus the cone's "
                             f"(1 - m) (N - 1) / 2), its meta-pupil leaves {limit} (margin c = {int(c)}; build the env with a larger "
                             "meta_pupil_pixels)")


def install_layer_sum_cone(front, layers, mirrors, geometry, coeff=None):
    """``conjugate.install_layer_sum_conjugate`` for a source at finite range (``aog_install_layer_sum_cone``, include/aogym_cone.h):
    ``geometry`` [L + n_mirrors, B, 3] float64 host array of (sx, sy, m), the layers' first (``cone_geometry``); ``mirrors`` may be empty.
    Stream-ordered, no host synchronisation."""
    n = len(layers) + len(mirrors)
    geometry = np.ascontiguousarray(geometry, dtype=np.float64)
    if geometry.shape != (n, front.num_envs, 3):
        raise ValueError(f"install_layer_sum_cone: geometry must be [{n}, {front.num_envs}, 3], got {geometry.shape}")
    handles = (C.c_void_p * max(1, len(mirrors)))(*[m._handle.value for m in mirrors])
    front._install_layers(front.lib.aog_install_layer_sum_cone, layers, handles, len(mirrors), C.c_void_p(geometry.ctypes.data), terms=True, coeff=coeff,
                          coeff_optional=True)


def resolve_sightline(spec, num_envs, total_envs=None, global_env_offset=0, name="sightline"):
    """One entry of ``sightlines``: an angle ((theta_x, theta_y) or per-env pairs), or dict(angle=, range=) for a source at finite range.
    Returns (angle [B, 2], range [B])."""
    rng = None
    if isinstance(spec, dict):
        if not set(spec) <= {"angle", "range"} or "angle" not in spec:
            raise ValueError(f"{name}: a dict with 'angle' and, optionally, 'range'")
        spec, rng = spec["angle"], spec.get("range")
    return (resolve_field_angle(spec, num_envs, total_envs, global_env_offset, name),
            resolve_range(rng, num_envs, total_envs, global_env_offset, f"{name}: range"))


def install_layer_sum_sightline(front, layers, shifts, coeff=None):
    """``BatchedAOEnv.install_layer_sum`` along a line of sight (``aog_install_layer_sum_sightline``, include/aogym_sightline.h): ``front`` a
    quasi-static env with N pixels, ``layers`` 1 .. 8 dynamic envs of N_l >= N pixels (N_l - N even) of its batch and device, ``shifts``
    [L, B, 2] float64 host array of (sx, sy) in pixels, |s| <= (N_l - N) / 2 - 1.  ``coeff``: None, or the [B, K] float64 device tensor of
    ``install_layer_sum_disturbed`` (the front holds a basis of K terms).  Stream-ordered, no host synchronisation."""
    shifts = np.ascontiguousarray(shifts, dtype=np.float64)
    if shifts.shape != (len(layers), front.num_envs, 2):
        raise ValueError(f"install_layer_sum_sightline: shifts must be [{len(layers)}, {front.num_envs}, 2], got {shifts.shape}")
    front._install_layers(front.lib.aog_install_layer_sum_sightline, layers, C.c_void_p(shifts.ctypes.data), terms=True, coeff=coeff, coeff_optional=True)


class Sightline:
    """A second line of sight through a ``LayeredAOEnv``'s layers (``LayeredAOEnv.add_sightline``): a quasi-static front of its own that
    gets the same layers' sum installed at its own shifts every step and steps with the env's action.  ``env`` is that front, an ordinary
    ``BatchedAOEnv``, for instruments (``wavefront_truth``, the science camera, ...); ``angle`` [B, 2] radians; ``last`` the dict of its
    last step (what ``info["sightlines"][name]`` carries); ``range`` [B] metres, the distance of what it looks at (inf: a plane wave), fixed
    when it is added."""

    def __init__(self, owner, name, env, angle, range=None):
        self._owner, self.name, self.env, self.angle = owner, name, env, angle
        self.range = np.full(len(angle), np.inf) if range is None else range
        self.last = None

    def set_angle(self, angle):
        """Point this sightline elsewhere (inside the meta-pupil's margin: ``ValueError`` otherwise, before anything changes).  The next
        installation — the next step, or ``reset`` — reads the layers there."""
        self._look(*self._owner._shifts_for(angle, f"sightline {self.name!r}", self.range))

    def _look(self, angle, shifts, geometry=None):
        """Store a checked line of sight (``LayeredAOEnv._shifts_for``): the next installation reads the layers at ``shifts`` — from a finite
        range through ``geometry`` [S, B, 3], which is None when every magnification is 1 (the plane-wave installation)."""
        self.angle, self._shifts, self._geometry = angle, shifts, geometry


class _InstalledFront(BatchedAOEnv):
    """A front whose screens are installed, never drawn: the ``LayeredAOEnv``'s own and the front of every ``Sightline``."""

    def _generate_screens(self, mask=None):
        """The front draws no screens: its layers do (at construction and in ``set_turbulence``)."""

    def _push_turbulence(self):
        """Nor does its handle need the per-env Cn^2 (only screen synthesis and the extrusion read them)."""

    def _host_extrusion_noise(self):
        """The layers draw their own normals (``evolve_atmosphere``)."""


class LayeredAOEnv(_InstalledFront):
    """``BatchedAOEnv`` over a layered dynamic atmosphere.  Keywords as ``BatchedAOEnv`` (``atm_type`` is 'dynamic'; ``atm_vel`` and
    ``screens`` do not apply) plus

    atm_layers   [{"fraction": f_l, "speed": v_l}, ...], 1 .. 8 layers (``resolve_layers``); ``atm_fried`` is the r0 of their sum.
    disturbance  None, or dict(shapes=, vibrations=, static=) for a ``disturbance.ModalDisturbance``: vibration lines and static
                 aberrations on K <= 8 pupil shapes, advanced once per step and added inside the layer sum (so everything that reads the
                 front sees them).  ``env.disturbance`` is the object; ``get_state`` / ``set_state`` carry its state; ``set_turbulence`` and
                 ``reset`` leave it alone.  Without it the env runs exactly the launches it ran before.
    layer_altitudes   None (every layer in the pupil plane: the env constructs and launches exactly what it did before), or [h_l] in
                 metres, one per layer, each >= 0.
    field_angle  the env's own line of sight, (theta_x, theta_y) in radians — one pair, or per-env pairs [B, 2] (or [total_envs, 2]
                 indexed by global env id).  Default on axis.  Needs ``layer_altitudes``.
    meta_pupil_pixels   N_L, the side of the meta-pupil the layers above the ground are drawn on (``N_L - N`` even, >= 0).  Default
                 (``default_meta_pupil_pixels``): the smallest accepted size that leaves the margin c >= ceil(max |h_l theta| /
                 pupil_pixel) + 1 over every sightline declared at construction (``field_angle`` and ``sightlines``).
    sightlines   None, or {name: angle} — ``add_sightline(angle, name)`` for each at the end of construction, counted in the default margin.
                 An entry may be ``dict(angle=(tx, ty), range=9e4)`` instead: that sightline looks at a source at finite range.
    source_range None or inf (a plane wave: the env constructs and launches exactly what it did before), or the distance in metres of
                 what the env's own front looks at — a laser guide star, an aircraft or satellite terminal — a scalar or per-env values
                 ([B] / [total_envs], ``resolve_per_env``).  Needs ``layer_altitudes``.  Light from range H crosses a source at altitude h
                 inside a cone: the front reads the layer's (and altitude mirror's) footprint shrunk by m = 1 - h / H about the point its
                 angle selects (``cone_geometry``, ``aog_install_layer_sum_cone``).  Every layer and mirror must lie below the source
                 (``ValueError`` naming it); the default margin counts the (1 - m) (N - 1) / 2 pixels the footprint's far edge moves.
                 Ranges are fixed at construction (the env's, and each sightline's at ``add_sightline(angle, name, range=)``);
                 ``get_state`` records them and ``set_state`` refuses a state taken with others.  A front all of whose magnifications are 1
                 takes the plane-wave installation, bit for bit what it took before.  Not modelled: the spherical wave's amplitude, a laser
                 spot's elongation, focus indetermination, a range that changes during an episode.
    altitude_mirrors   None (the env constructs and launches exactly what it did before), or [dict(altitude=h, actuators=9), ...] —
                 ``conjugate.resolve_mirror``'s forms — for one ``conjugate.AltitudeMirror`` each: ``env.altitude_mirrors`` is the list.  Needs
                 ``layer_altitudes``; layers plus mirrors are at most 8; the mirrors' altitudes count in the default margin and in every
                 margin check (construction, ``add_sightline``, ``set_angle``, ``set_field_angle``).  Every front — the env's own and each
                 sightline's — gets the mirrors' surfaces installed beside the layers at its own ``h_m theta / pupil_pixel``
                 (``aog_install_layer_sum_conjugate``).  A mirror is absolute, like the pupil mirror: a command
                 (``env.altitude_mirrors[j].set_command``) stands until it is set again and shows in the next installation (the next
                 ``step``).  ``reset(mask)`` with ``flat_mirror_start_per_episode`` zeroes the masked envs' commands and installs again;
                 ``get_state`` / ``set_state`` carry the commands; ``close`` closes the mirrors.  There is no servo on the altitude mirrors:
                 a command acts in full on the step it precedes.
    altitude_action    None, or a scale: ``action_space`` (and ``single_action_space``) widen by the mirrors' mode counts, ``step`` takes
                 [B, A + sum K_m] actions, sets ``scale x`` the tail as the mirrors' commands (in mirror order, float64) before the layers
                 advance and steps with the head; ``info["altitude_commands"]`` is the list of what was set.  With it ``step_with_policy``,
                 ``step_with_spgd`` and ``step(next_actions=...)`` raise ``RuntimeError`` (the fused forms form or hold the action inside
                 a launch, where there is nothing to split); ``rollout()`` runs its unfused loop.
    scintillation   None (the env constructs and launches exactly what it did before), True or dict(guard=, scratch_bytes=): every layer
                 above the ground is propagated to the pupil by the weak-turbulence (Rytov) filter (``scintillation.py``,
                 ``aog_scint_filter``) after the layers evolve: every front's phase becomes the sum of the DIFFRACTED phases S_l (the
                 corrections S_l - phi_l are installed beside the layers like altitude mirrors' surfaces) and gets a log-amplitude map
                 chi = sum chi_l (``log_amplitude()``).  After every ``step`` the amplitude-aware receiver (``aog_scint_receive``) adds
                 ``info["scintillation"] = dict(power, irradiance, strehl, sigma_chi2)`` ([B] float64), and the same dict under
                 ``info["sightlines"][name]``.  ``info["power"]``, ``obs`` and ``reward`` stay the step's: the diffracted phase at unit
                 amplitude.  Needs ``layer_altitudes``; plane waves only (``source_range`` or a sightline ``range`` raise ``ValueError``);
                 layers plus mirrors plus filtered layers are at most 8 sources; the meta-pupil's margin grows by the guard band (default
                 ``scintillation.default_guard``: one Fresnel zone of the highest layer) and a too-small ``meta_pupil_pixels`` raises.
                 ``rytov_variance()`` is the theoretical sigma_chi^2 of the profile; <~ 0.3 is the filter's regime.  The fused and
                 pipelined step forms raise ``RuntimeError``; ``get_state`` / ``set_state`` carry nothing new (chi is a function of the
                 layers' screens).  An env whose layers all sit at h = 0 filters nothing: its step is bit for bit the step without the
                 option, and the receiver reports irradiance 1.
    servo        as ``BatchedAOEnv``'s (through ``**kw``): one mirror, one servo — the env's own front steps with ``servo.apply(actions)`` and
                 every sightline's front with the same applied action; the sightline fronts get no servo of their own.

    Layered geometry.  A layer at altitude 0 keeps N pixels and this env's tables; a layer above is built with
    ``dataclasses.replace(params, num_pupil_pixels=N_L, telescope_diameter=D N_L / N)`` — the same pixel pitch and Cn^2 on a wider
    screen, with tables of its own (shared among the layers of one size).  Layer l is read ``h_l theta / pupil_pixel`` pixels along the
    angle (``sightline_shifts``), bilinearly: whole-pixel shifts are exact translations, fractional ones attenuate the highest spatial
    frequencies (per axis by ``|1 - f + f exp(-i w)|`` at w radians per pixel: nothing at the scales r0 and the actuators resolve, up to
    all of it at the grid's Nyquist frequency).  ``add_sightline(angle, name)`` returns a ``Sightline``: a second quasi-static front built
    like the env's own (tables, ``act_type``, ``obs_dim``, reward, detector settings, global env ids, seed).  In every ``step`` the layers
    evolve once, every front gets the sum installed at its own shifts — the disturbance's coefficients are common-path, the same for all —
    the env's front steps, then every sightline's front steps with the same action; ``info["sightlines"][name]`` carries that front's
    ``obs``, ``reward``, ``power`` and ``strehl``.  ``reset`` resets them together, ``get_state`` / ``set_state`` carry them (angles
    included), ``close`` closes them; ``set_field_angle`` / ``Sightline.set_angle`` move a line of sight inside the margin.  A point-ahead
    study observes and controls on the beacon (the env) and reads power and fades on ``add_sightline((theta_pa, 0), "uplink")``, e.g.
    ``LinkTelemetry.push(info["sightlines"]["uplink"]["power"])``.  With sightlines attached ``step_with_policy`` / ``step_with_spgd`` raise
    ``RuntimeError``: fused policy stepping hands no action back before the step has run, so there is nothing to step the other fronts
    with; ``rollout()`` needs no new option — its unfused loop (``fused_policy=False``) goes through ``step``.

    Layer l is a private dynamic env with a seed of its own (``layer_seed``) and therefore wind directions and stencil draws of its own,
    as the reference draws them per layer; it shares this env's tables, ``extrusion``, ``screen_source`` and global env ids.  ``reset`` is
    the front's (the atmosphere is observed as it stands, like the reference's dynamic reset); ``step`` / ``step_with_policy`` first evolve
    every layer and install their sum, then step the front.  ``get_screens()`` is the float64 sum, ``layer_screens(l)`` one layer;
    ``velocity_vectors`` is [L, B, 2]; ``set_turbulence`` splits the new r0 by the same fractions; ``get_state`` / ``set_state`` carry the
    front's state and every layer's.  ``lookahead`` is not available (returns False) and ``set_screens`` raises.  ``obs_gradient`` goes to the
    front, an ordinary static handle: ``output_gradient`` differentiates the observation of the installed sum."""

    def __init__(self, num_envs=1, device=None, atm_layers=None, atm_fried=0.15, act_type="num_actuators", act_dim=64, obs_dim=2,
                 rew_type="strehl_ratio", rew_threshold=None, timesteps_per_episode=20, flat_mirror_start_per_episode=True, SH_operation=False, *,
                 atm_type="dynamic", seed=None, screen_source="device", rng=None, global_env_offset=0, total_envs=None, extrusion="auto",
                 verbose=True, disturbance=None, layer_altitudes=None, field_angle=None, meta_pupil_pixels=None, sightlines=None, altitude_mirrors=None,
                 altitude_action=None, source_range=None, scintillation=None, **kw):
        self._layers = []
        self.scintillation = None
        self.scintillation_on = False
        self._scint_cache = {}
        self._mirrors = []
        self._altitude_scale = None
        self._handle = None
        self.disturbance = None
        self._sightlines = {}
        self._altitudes = None
        self.source_range = None
        if atm_type != "dynamic":
            raise ValueError("LayeredAOEnv: atm_type is 'dynamic' (a layered atmosphere evolves every step)")
        for bad in ("atm_vel", "screens"):
            if bad in kw:
                raise ValueError(f"LayeredAOEnv: {bad} does not apply (every layer has its own speed and draws its own screens)")
        plan = resolve_layers(atm_layers, atm_fried, int(num_envs), total_envs, int(global_env_offset))
        # the geometry, checked before anything is created
        altitudes = resolve_altitudes(layer_altitudes, len(plan))
        if altitudes is None and (field_angle is not None or meta_pupil_pixels is not None or sightlines):
            raise ValueError("LayeredAOEnv: field_angle, meta_pupil_pixels and sightlines need layer_altitudes (without altitudes every layer sits "
                             "in the pupil plane and every direction sees the same wavefront)")
        if altitudes is None and source_range is not None:
            raise ValueError("LayeredAOEnv: source_range needs layer_altitudes (a source's range only shows through layers above the ground)")
        if altitudes is None and altitude_mirrors:
            raise ValueError("LayeredAOEnv: altitude_mirrors need layer_altitudes (a mirror conjugated to an altitude is drawn on the layers' meta-pupil)")
        from .scintillation import resolve_scintillation

        scint = resolve_scintillation(scintillation)
        if scint is not None and altitudes is None:
            raise ValueError("LayeredAOEnv: scintillation needs layer_altitudes (a layer in the pupil plane does not diffract)")
        if altitude_action is not None and not altitude_mirrors:
            raise ValueError("LayeredAOEnv: altitude_action needs altitude_mirrors")
        if altitude_action is not None and not np.isfinite(float(altitude_action)):
            raise ValueError(f"altitude_action: a finite scale, got {altitude_action!r}")
        geometry = None
        if altitudes is not None:
            from .conjugate import MAX_SOURCES, mirror_altitude, resolve_mirror
            from .params import OpticalParams

            mirror_specs = list(altitude_mirrors or ())
            if len(plan) + len(mirror_specs) > MAX_SOURCES:
                raise ValueError(f"LayeredAOEnv: {len(plan)} layers and {len(mirror_specs)} altitude mirrors: an installation reads at most "
                                 f"{MAX_SOURCES} sources")
            # (the altitudes of every source an installation reads: the layers', then the mirrors')
            seen_at = np.concatenate([altitudes, [mirror_altitude(m) for m in mirror_specs]]) if mirror_specs else altitudes

            params = kw.get("params") or OpticalParams(num_pupil_pixels=int(kw.get("num_pupil_pixels", 240)))
            n_env, n_off = int(num_envs), int(global_env_offset)
            angle = resolve_field_angle(field_angle, n_env, total_envs, n_off)
            if sightlines is not None and not isinstance(sightlines, dict):
                raise ValueError("sightlines: a dict {name: angle}")
            own_range = resolve_range(source_range, n_env, total_envs, n_off)
            looks = {str(k): resolve_sightline(v, n_env, total_envs, n_off, f"sightline {k!r}") for k, v in (sightlines or {}).items()}
            declared = {k: a for k, (a, _) in looks.items()}
            N = params.num_pupil_pixels
            every = [("field_angle", angle, own_range)] + [(f"sightline {k!r}", a, H) for k, (a, H) in looks.items()]
            # The ranges as declared, for every env of the whole batch: what is refused and how large the default meta-pupil is must not
            # depend on which envs this instance holds.  (With every source at infinity the margin is the plane wave's own, as it was.)
            stated = [declared_range(source_range)] + [declared_range(v.get("range") if isinstance(v, dict) else None) for v in (sightlines or {}).values()]
            finite = any(np.any(np.isfinite(H)) for H in stated)
            guard = 0
            if scint is not None:
                from .scintillation import default_guard

                if finite:
                    raise ValueError("LayeredAOEnv: scintillation models plane waves only; source_range or a sightline's range does not go with it "
                                     "(the spherical wave's scaling of the Fresnel filter is not built)")
                filtered = int(np.count_nonzero(altitudes > 0))
                if len(plan) + len(mirror_specs) + filtered > MAX_SOURCES:
                    raise ValueError(f"LayeredAOEnv: {len(plan)} layers, {len(mirror_specs)} altitude mirrors and the diffraction corrections of {filtered} "
                                     f"layers above the ground: an installation reads at most {MAX_SOURCES} sources")
                guard = default_guard(altitudes, params.wavelength_wfs, params.pupil_pixel) if scint["guard"] is None else (scint["guard"] if filtered else 0)
            if finite:
                for (what, _, _), H in zip(every, stated):   # (a layer or mirror at or above a source, before anything else)
                    cone_geometry(seen_at, np.zeros((H.size, 2)), H, params.pupil_pixel, first_mirror=len(plan), what=what)
            if meta_pupil_pixels is None:
                n_meta = default_meta_pupil_pixels(N, required_margin_cone(seen_at, [(a, H) for (_, a, _), H in zip(every, stated)], params.pupil_pixel, N)
                                                   if finite else required_margin(seen_at, [angle] + list(declared.values()), params.pupil_pixel, guard))
            else:
                n_meta = int(meta_pupil_pixels)
                if n_meta != meta_pupil_pixels or n_meta < N or (n_meta - N) % 2:
                    raise ValueError(f"meta_pupil_pixels: expected an integer >= num_pupil_pixels ({N}) with an even difference, got {meta_pupil_pixels!r}")
            margins = np.where(seen_at > 0, (n_meta - N) // 2, 0)
            if guard and (n_meta - N) // 2 < guard + 1:
                raise ValueError(f"meta_pupil_pixels: {n_meta} leaves a margin of {(n_meta - N) // 2} pixels, the scintillation's guard band alone takes "
                                 f"{guard} (and a sightline at least 1 more)")
            true_margins, margins = margins, np.where(seen_at > 0, (n_meta - N) // 2 - guard, 0)   # (what a shift may use: the guard stays clear)
            for what, a, H in every:
                if np.any(np.isfinite(H)):
                    check_margin_cone(cone_geometry(seen_at, a, H, params.pupil_pixel, first_mirror=len(plan), what=what), margins, N, what,
                                      first_mirror=len(plan))
                else:
                    check_margin(sightline_shifts(seen_at, a, params.pupil_pixel), margins, what, first_mirror=len(plan))
            for m in mirror_specs:
                resolve_mirror(m, N, n_meta)   # (actuators, coupling and a given basis's shape)
            geometry = dict(angle=angle, declared=looks, n_meta=n_meta, margins=true_margins[:len(plan)], seen_at=seen_at, seen_margins=margins,
                            mirrors=mirror_specs, range=own_range, guard=guard)
        self._front_args = dict(args=(act_type, act_dim, obs_dim, rew_type, rew_threshold, timesteps_per_episode, flat_mirror_start_per_episode,
                                      SH_operation), seed=seed, extrusion=extrusion, kw={k: v for k, v in kw.items() if k != "servo"})   # (one mirror, one servo: the env's)
        # The front: a quasi-static handle whose screens are installed, never drawn (_InstalledFront); it consumes no
        # host random draws, so layer 0 sees the streams a plain dynamic env with the same seed sees.
        super().__init__(num_envs, device, "quasi_static", 0, atm_fried, act_type, act_dim, obs_dim, rew_type, rew_threshold, timesteps_per_episode,
                         flat_mirror_start_per_episode, SH_operation, seed=seed, screen_source="device", rng=None,
                         global_env_offset=global_env_offset, total_envs=total_envs, extrusion=extrusion, verbose=verbose, **kw)
        self.atm_type = "dynamic"
        self.screen_source = screen_source
        self.layer_fractions = np.array([p["fraction"] for p in plan])
        layer_kw = {k: kw[k] for k in ("screen_oversampling", "precision", "kernel", "pixel_chunks", "screen_method") if k in kw}
        try:
            meta_params = meta_tables = None
            for i, p in enumerate(plan):
                lay_params, lay_tables = self.params, self.tables
                if geometry is not None and geometry["margins"][i] > 0:
                    # a layer above the ground on the meta-pupil: the same pitch (and with it the same Cn^2 per r0) on a wider screen
                    if meta_params is None:
                        N, n_meta = self.num_pupil_pixels, geometry["n_meta"]
                        meta_params = dataclasses.replace(self.params, num_pupil_pixels=n_meta, telescope_diameter=self.params.telescope_diameter * n_meta / N)
                    lay_params, lay_tables = meta_params, meta_tables
                # (timesteps_per_episode = 0: a layer is never reset, and the int8 extrusion only works ahead inside an episode)
                self._layers.append(BatchedAOEnv(self.num_envs, self.device, "dynamic", p["speed"], p["fried"], act_type, act_dim, obs_dim, rew_type,
                                                 None, 0, True, False, params=lay_params, seed=layer_seed(seed, i), screen_source=screen_source,
                                                 rng=rng, global_env_offset=self.global_env_offset, total_envs=self.total_envs,
                                                 tables=lay_tables, extrusion=extrusion, verbose=False, **layer_kw))
                if lay_params is meta_params:
                    meta_tables = self._layers[-1].tables
            self.velocity_vectors = np.stack([lay.velocity_vectors for lay in self._layers])   # [L, B, 2] m/s
            self.velocity = [lay.velocity for lay in self._layers]
            if disturbance is not None:
                self._attach_disturbance(disturbance)
            if geometry is not None:
                self._altitudes = altitudes
                self.meta_pupil_pixels = geometry["n_meta"]
                self.layer_margins = geometry["margins"]          # [L] c_l: the meta-pupil's margin on every side, 0 for a ground layer
                self.field_angle = geometry["angle"]              # [B, 2] radians
                self._seen_at, self._seen_margins = geometry["seen_at"], geometry["seen_margins"]   # the layers', then the mirrors'
                self.source_range = geometry["range"]             # [B] metres, inf: a plane wave; fixed at construction
                self._look(*self._shifts_for(self.field_angle, "field_angle", self.source_range))
                if geometry["mirrors"]:
                    from .conjugate import AltitudeMirror

                    for m in geometry["mirrors"]:
                        self._mirrors.append(AltitudeMirror(self, **m))
                    if altitude_action is not None:
                        from .spaces import make_box

                        self._altitude_scale = float(altitude_action)
                        width = self.num_modes + sum(m.n_modes for m in self._mirrors)
                        self.action_space = self.single_action_space = make_box(-1, 1, (width,), np.float16)
            if scint is not None:
                from .scintillation import Scintillation

                if kw.get("precision", "fast") != "fast":
                    raise ValueError("LayeredAOEnv: scintillation needs a fast front (its log-amplitude map and receiver are built on the screen tiles)")
                self.scintillation_guard = geometry["guard"]
                self.scintillation = Scintillation(self, [i for i, h in enumerate(altitudes) if h > 0], scint["scratch_bytes"])
                self.scintillation_on = True
                self._chi_tile = self.scintillation.tile(self)
                self._filter()
            self._install()   # the first reset sees t = 0
            if geometry is not None:
                for name, (angle, rng) in geometry["declared"].items():
                    self.add_sightline(angle, name, rng)
        except Exception:
            self.close()
            raise

    num_layers = property(lambda self: len(self._layers))

    @property
    def wind_speeds(self):
        """[L, B] float64 wind speed of every layer and env."""
        return np.stack([lay.wind_speeds for lay in self._layers])

    def _attach_disturbance(self, disturbance):
        """``disturbance``: dict(shapes=, vibrations=, static=[, seed=]) for a ``ModalDisturbance`` of this env, or such an object made for
        this env's batch, global env ids and device.  Its basis goes to the front; from here on every installation is the disturbed form."""
        from .disturbance import ModalDisturbance

        if isinstance(disturbance, dict):
            if not set(disturbance) <= {"shapes", "vibrations", "static", "seed"} or "shapes" not in disturbance:
                raise ValueError("disturbance: a dict with 'shapes' and, optionally, 'vibrations', 'static' and 'seed'")
            disturbance = ModalDisturbance(self, **disturbance)
        elif not isinstance(disturbance, ModalDisturbance):
            raise ValueError("disturbance: a dict(shapes=, vibrations=, static=) or a ModalDisturbance")
        d = disturbance
        index = self.device.index if self.device.index is not None else self._torch.cuda.current_device()
        if d.device.index != index or d.num_envs != self.num_envs or d.global_env_offset != self.global_env_offset:
            raise ValueError(f"disturbance: made for {d.num_envs} envs from global id {d.global_env_offset} on {d.device}, this env has "
                             f"{self.num_envs} from {self.global_env_offset} on {self.device}")
        if d.basis.shape[1] != int(self.tables.n_ap):
            raise ValueError(f"disturbance: its shapes cover {d.basis.shape[1]} aperture pixels, this env's pupil has {int(self.tables.n_ap)}")
        d.upload_basis(self)
        self.disturbance = d
        self._coeff = d.coefficients()

    def _install_front(self, front, shifts, coeff, geometry=None):
        """One front's installation along its line of sight: the layers, and the altitude mirrors' surfaces when the env has any.  Only a
        front that looks at a source at finite range (``geometry``: some m < 1) takes the cone form; every other front calls what it called
        before there were ranges."""
        if geometry is not None:
            install_layer_sum_cone(front, self._layers, self._mirrors, geometry, coeff)
        elif self.scintillation is not None and self.scintillation.corrections:
            # the diffraction corrections S_l - phi_l as further sources behind the layers and mirrors, each at its layer's shift: the
            # front's phase is sum S_l; then the front's log-amplitude map from the chi_l at the same shifts
            from .conjugate import install_layer_sum_conjugate

            extended, own, own_dev = self._scint_shifts(shifts)
            install_layer_sum_conjugate(front, self._layers, self._mirrors + self.scintillation.corrections, extended, coeff)
            self.scintillation.install(front, own, own_dev, front._chi_tile)
        elif self._mirrors:
            from .conjugate import install_layer_sum_conjugate

            install_layer_sum_conjugate(front, self._layers, self._mirrors, shifts, coeff)
        else:
            install_layer_sum_sightline(front, self._layers, shifts, coeff)

    def _scint_shifts(self, shifts):
        """(``shifts`` with the filtered layers' rows appended, those rows alone, the same on the device), kept per shifts array so that
        a step builds and copies nothing."""
        hit = self._scint_cache.get(id(shifts))
        if hit is None or hit[0] is not shifts:
            if len(self._scint_cache) >= 16:
                self._scint_cache.clear()
            own = np.ascontiguousarray(shifts[self.scintillation.layer_index])
            hit = (shifts, np.ascontiguousarray(np.concatenate([shifts, own])), own, self._torch.from_numpy(own).to(self.device))
            self._scint_cache[id(shifts)] = hit
        return hit[1:]

    def _filter(self):
        """The Fresnel filter of the layers' current screens: after they evolve or are redrawn, before an installation."""
        if self.scintillation is not None:
            self.scintillation.filter()

    def _refuse_with_scintillation(self, who):
        if self.scintillation_on:
            raise RuntimeError(f"{who}: this env has scintillation on; its receiver reads the mirror after every step, where {who} already holds the "
                               "next action — use step(), or rollout(fused_policy=False)")

    def _receive(self, front):
        """The amplitude-aware receiver's dict for ``front`` in its current state."""
        return self.scintillation.receive(front, front._chi_tile if self.scintillation.corrections else None)

    def log_amplitude(self, first=0, count=None):
        """[count, N, N] float32: the log-amplitude chi (nepers) on the env's own pupil as last installed, zeros outside the aperture."""
        if not self.scintillation_on:
            raise RuntimeError("log_amplitude: this env was built without scintillation")
        return self.scintillation.unpack_tile(self, self._chi_tile, first, count)

    def rytov_variance(self):
        """[B] float64: the theoretical log-amplitude variance sigma_chi^2 of the configured profile per env (``scintillation.rytov_variance``
        on the filter's own grid, with ``atm_fried`` taken at the science wavelength as the screens take it); <~ 0.3 is the regime of the
        weak-turbulence filter."""
        from .scintillation import rytov_variance

        if not self.scintillation_on:
            raise RuntimeError("rytov_variance: this env was built without scintillation")
        return rytov_variance(self._altitudes, self.layer_fractions, self._fried, self.params.wavelength_wfs, self.params.pupil_pixel,
                              (self.meta_pupil_pixels,) * 2, 0, self.params.outer_scale, fried_wavelength=self.params.wavelength_sci)

    def _install(self):
        coeff = None if self.disturbance is None else self._coeff
        if self._altitudes is not None:
            # every front reads the same layers (and mirrors) at its own shifts; the coefficients are common-path
            self._install_front(self, self._shifts, coeff, self._geometry)
            for sl in self._sightlines.values():
                self._install_front(sl.env, sl._shifts, coeff, sl._geometry)
        elif coeff is None:
            self.install_layer_sum(self._layers)
        else:
            self.install_layer_sum_disturbed(self._layers, coeff)

    layer_altitudes = property(lambda self: None if self._altitudes is None else self._altitudes.copy(), doc="[L] metres, or None")
    sightlines = property(lambda self: dict(self._sightlines), doc="{name: Sightline}")
    altitude_mirrors = property(lambda self: list(self._mirrors), doc="[conjugate.AltitudeMirror], in the order of ``altitude_mirrors=``")

    def _shifts_for(self, angle, what, rng=None):
        """``angle`` resolved to [B, 2], its shifts [L, B, 2] and, for a source at ``rng`` [B] metres with some magnification below 1, the
        geometry [L, B, 3] (None otherwise), checked against the margins (``ValueError`` before anything changes)."""
        if self._altitudes is None:
            raise ValueError(f"{what}: this env was built without layer_altitudes (every layer sits in the pupil plane and every direction sees "
                             "the same wavefront)")
        angle = resolve_field_angle(angle, self.num_envs, self.total_envs, self.global_env_offset, what)
        if rng is not None and np.any(np.isfinite(rng)):
            geometry = cone_geometry(self._seen_at, angle, rng, self.params.pupil_pixel, first_mirror=len(self._layers), what=what)
            check_margin_cone(geometry, self._seen_margins, self.num_pupil_pixels, what, first_mirror=len(self._layers))
            shifts = np.ascontiguousarray(geometry[:, :, :2])
            return angle, shifts, (geometry if np.any(geometry[:, :, 2] != 1.0) else None)
        shifts = sightline_shifts(self._seen_at, angle, self.params.pupil_pixel)
        check_margin(shifts, self._seen_margins, what, first_mirror=len(self._layers))
        return angle, shifts, None

    def add_sightline(self, angle, name=None, range=None):
        """A second front over the same layers that looks along ``angle`` ((theta_x, theta_y) radians, or per-env pairs) at a source
        ``range`` metres away (a scalar or per-env values; None or inf: a plane wave, whatever the env's own ``source_range``): returns its
        ``Sightline``.  ``ValueError`` when the angle leaves the meta-pupil's margin, a layer or mirror lies at or above the source or the
        name is taken, before anything is created."""
        name = f"sightline{len(self._sightlines)}" if name is None else str(name)
        if name in self._sightlines:
            raise ValueError(f"add_sightline: there is a sightline {name!r} already")
        rng = resolve_range(range, self.num_envs, self.total_envs, self.global_env_offset, f"sightline {name!r}: range")
        if self.scintillation_on and np.any(np.isfinite(rng)):
            raise ValueError(f"sightline {name!r}: scintillation models plane waves only; a range does not go with it")
        angle, shifts, geometry = self._shifts_for(angle, f"sightline {name!r}", rng)
        fa = self._front_args
        front = _InstalledFront(self.num_envs, self.device, "quasi_static", 0, self.fried_parameter, *fa["args"], seed=fa["seed"], screen_source="device",
                                rng=None, global_env_offset=self.global_env_offset, total_envs=self.total_envs, extrusion=fa["extrusion"],
                                verbose=False, **{**fa["kw"], "tables": self.tables, "params": self.params})
        try:
            if self.disturbance is not None:
                self.disturbance.upload_basis(front)
            if self.scintillation_on:
                front._chi_tile = self.scintillation.tile(front)
            sl = Sightline(self, name, front, angle, rng)
            sl._look(angle, shifts, geometry)
            self._install_front(front, shifts, None if self.disturbance is None else self._coeff, geometry)
        except Exception:
            front.close()
            raise
        self._sightlines[name] = sl
        return sl

    def set_field_angle(self, angle):
        """Point the env's own line of sight elsewhere (inside the meta-pupil's margin: ``ValueError`` otherwise, before anything changes).
        The next installation — the next step — reads the layers there."""
        self._look(*self._shifts_for(angle, "field_angle", self.source_range))

    def _look(self, angle, shifts, geometry=None):
        """``Sightline._look`` for the env's own line of sight."""
        self.field_angle, self._shifts, self._geometry = angle, shifts, geometry

    def _refuse_with_sightlines(self, who):
        if self._sightlines:
            raise RuntimeError(f"{who}: this env has sightlines attached ({', '.join(self._sightlines)}); fused stepping hands no action back before "
                               "the step has run, so their fronts cannot be stepped with it — use step(), or rollout(fused_policy=False)")

    def _refuse_with_altitude_action(self, who):
        if self._altitude_scale is not None:
            raise RuntimeError(f"{who}: this env splits its action between the pupil mirror and the altitude mirrors (altitude_action); {who} forms or "
                               "holds the action inside a launch, where there is nothing to split — use step(), or rollout(fused_policy=False)")

    def _flatten_altitude_mirrors(self, mask):
        """The masked envs' altitude mirrors start the episode flat (``flat_mirror_start_per_episode``), installed before the reset observes."""
        if self._mirrors and self.flat_mirror_start_per_episode:
            for m in self._mirrors:
                m.set_command(self._torch.zeros((self.num_envs, m.n_modes), dtype=self._torch.float64, device=self.device), mask)
            self._install()

    def install_layer_sum_disturbed(self, layers, coeff):
        """``install_layer_sum`` with ``sum_k coeff[b][k] shape_k`` added inside the float64 sum (``aog_install_layer_sum_disturbed``; the
        shapes are those last uploaded with ``ModalDisturbance.upload_basis``).  ``coeff``: [B, K] float64 device tensor, metres of optical path."""
        self._install_layers(self.lib.aog_install_layer_sum_disturbed, layers, terms=True, coeff=coeff)

    def _advance(self):
        for lay in self._layers:
            lay.evolve_atmosphere()
        if self.disturbance is not None:
            self._coeff = self.disturbance.advance()
        self._filter()
        self._install()

    def step(self, actions, out=None, next_actions=BatchedAOEnv._PIPELINE_END):
        if next_actions is not BatchedAOEnv._PIPELINE_END:
            self._refuse_with_scintillation("step(next_actions=...)")
            self._refuse_with_altitude_action("step(next_actions=...)")
            self._refuse_with_servo("step(next_actions=...)", "step(actions), one call per step")   # (before the layers move)
        commands = None
        if self._altitude_scale is not None:
            # the tail of the action is the altitude mirrors', in mirror order: set before the layers advance, installed with them
            torch = self._torch
            widths = [self.num_modes] + [m.n_modes for m in self._mirrors]
            a = torch.as_tensor(actions, device=self.device)
            if a.dim() != 2 or tuple(a.shape) != (self.num_envs, sum(widths)):
                raise ValueError(f"step: actions must be [{self.num_envs}, {sum(widths)}] ({self.num_modes} for the pupil mirror, then "
                                 f"{widths[1:]} for the altitude mirrors), got {list(a.shape)}")
            actions, *tails = torch.split(a.to(torch.float32), widths, dim=1)
            actions = actions.contiguous()
            commands = [m.set_command(t.to(torch.float64) * self._altitude_scale) for m, t in zip(self._mirrors, tails)]
        self._advance()
        ret = super().step(actions, out=out, next_actions=next_actions)
        if commands is not None:
            ret[4]["altitude_commands"] = commands
        if self._sightlines:
            # (after the env's own front: every sightline's front takes the same action — with a servo the one the mirror received — on the
            # sum _advance installed at its shifts)
            seen = {}
            applied = ret[4].get("applied_action", actions)
            for name, sl in self._sightlines.items():
                obs, reward, _, _, info = sl.env.step(applied)
                sl.last = seen[name] = {"obs": obs, "reward": reward, "power": info["power"], "strehl": info["strehl"]}
                if self.scintillation_on:
                    seen[name]["scintillation"] = self._receive(sl.env)
            ret[4]["sightlines"] = seen
        if self.scintillation_on:
            ret[4]["scintillation"] = self._receive(self)
        return ret

    def reset(self, mask=None, seed=None, options=None):
        self._flatten_altitude_mirrors(mask)
        ret = super().reset(mask, seed, options)
        self._reset_sightlines(mask)
        return ret

    def _reset_sightlines(self, mask):
        for sl in self._sightlines.values():
            sl.env.reset(mask)
            sl.last = None

    def reset_with_policy(self, policy, cov_var=0.5, policy_out=None, mask=None, ou_noise=None, action_mode="sample"):
        self._flatten_altitude_mirrors(mask)
        ret = super().reset_with_policy(policy, cov_var, policy_out=policy_out, mask=mask, ou_noise=ou_noise, action_mode=action_mode)
        self._reset_sightlines(mask)
        return ret

    def reset_with_spgd(self, ctrl, mask=None, action_out=None):
        self._flatten_altitude_mirrors(mask)
        ret = super().reset_with_spgd(ctrl, mask=mask, action_out=action_out)
        self._reset_sightlines(mask)
        return ret

    def step_with_policy(self, policy, cov_var=0.5, out=None, policy_out=None, action=None, ou_noise=None, action_mode="sample"):
        self._refuse_with_scintillation("step_with_policy")
        self._refuse_with_altitude_action("step_with_policy")
        self._refuse_with_sightlines("step_with_policy")
        self._refuse_with_servo("step_with_policy", "step(policy(obs)), or rollout(fused_policy=False)")
        self._advance()
        return super().step_with_policy(policy, cov_var, out=out, policy_out=policy_out, action=action, ou_noise=ou_noise, action_mode=action_mode)

    def step_with_spgd(self, ctrl, out=None, action=None, action_out=None):
        self._refuse_with_scintillation("step_with_spgd")
        self._refuse_with_altitude_action("step_with_spgd")
        self._refuse_with_sightlines("step_with_spgd")
        self._refuse_with_servo("step_with_spgd", "step(ctrl.action()), or rollout(fused_policy=False)")
        self._advance()
        return super().step_with_spgd(ctrl, out=out, action=action, action_out=action_out)

    def evolve_atmosphere(self):
        raise RuntimeError("LayeredAOEnv: the layers evolve inside step()")

    def lookahead(self, enable=True):
        return False

    def set_screens(self, screens, first=0):
        raise RuntimeError("LayeredAOEnv: the screens are the sum of the layers'; there is nothing to install")

    def set_extrusion_noise(self, noise):
        raise RuntimeError("LayeredAOEnv: hand each layer its normals (env.layers[l].set_extrusion_noise)")

    @property
    def layers(self):
        """The layers' envs (read their ``velocity_vectors`` / ``get_screens()``, or hand one its extrusion normals; do not step them)."""
        return tuple(self._layers)

    def layer_screens(self, layer, first=0, count=None):
        """Current float64 master screens of one layer: [count, N, N]."""
        return self._layers[layer].get_screens(first, count)

    def get_screens(self, first=0, count=None):
        """The float64 sum of the layers' screens in layer order (what ``install_layer_sum`` forms before it removes the aperture mean).
        With ``layer_altitudes``: of the pupil-sized centres of the layers' meta-pupils — the sum an on-axis sightline reads."""
        N = self.num_pupil_pixels
        total = None
        for lay in self._layers:
            c = (lay.num_pupil_pixels - N) // 2
            part = lay.get_screens(first, count)
            part = part if c == 0 else part[:, c:c + N, c:c + N].contiguous()
            total = part if total is None else total + part
        return total

    def set_turbulence(self, fried, mask=None):
        """New total r0 for the envs ``mask`` selects: every layer gets r0 f_l^(-3/5) and redraws those envs' screens now."""
        fried, _, _ = resolve_per_env("fried", fried, self.num_envs, self.total_envs, self.global_env_offset)
        if np.any(fried <= 0):
            raise ValueError("set_turbulence: Fried parameters must be > 0")
        sel = _mask_array(mask, self.num_envs, "set_turbulence")
        new = self._fried.copy()
        new[sel] = fried[sel]
        self._apply_fried(new)   # (raises before any layer changed when r0 is below what the extrusion tables were made for)
        for lay, f in zip(self._layers, self.layer_fractions):
            lay.set_turbulence(new * f ** (-3.0 / 5.0), mask)
        self._filter()   # (the redrawn screens)
        self._install()

    def get_state(self):
        state = super().get_state()
        state["layers"] = [lay.get_state() for lay in self._layers]
        if self.disturbance is not None:
            state["disturbance"] = self.disturbance.state_dict()
        if self._altitudes is not None:
            state["field_angle"] = self.field_angle.copy()
            state["sightlines"] = {name: dict(angle=sl.angle.copy(), env=sl.env.get_state()) for name, sl in self._sightlines.items()}
            self._record_ranges(state)
        if self._mirrors:
            state["altitude_mirrors"] = [m.get_state() for m in self._mirrors]
        return state

    def _record_ranges(self, state):
        """The ranges' part of ``get_state``: recorded where there is one — a state without them is one of plane waves, as every state was
        before there were ranges."""
        if np.any(np.isfinite(self.source_range)):
            state["source_range"] = self.source_range.copy()
        for name, sl in self._sightlines.items():
            if np.any(np.isfinite(sl.range)):
                state["sightlines"][name]["range"] = sl.range.copy()

    def set_state(self, state):
        if len(state.get("layers", ())) != len(self._layers):
            raise ValueError("set_state: the state was saved with another number of layers")
        if ("disturbance" in state) != (self.disturbance is not None):
            raise ValueError("set_state: the state was saved " + ("with" if "disturbance" in state else "without") + " a disturbance, this env was built "
                             + ("without" if self.disturbance is None else "with") + " one")
        self._check_servo_state(state)   # (here too, before a layer is touched: super().set_state checks it again)
        if ("field_angle" in state) != (self._altitudes is not None) or set(state.get("sightlines", ())) != set(self._sightlines):
            raise ValueError(f"set_state: the state was saved with layer altitudes {'on' if 'field_angle' in state else 'off'} and the sightlines "
                             f"{sorted(state.get('sightlines', ()))}, this env has them {'on' if self._altitudes is not None else 'off'} and "
                             f"{sorted(self._sightlines)}")
        if len(state.get("altitude_mirrors", ())) != len(self._mirrors):
            raise ValueError(f"set_state: the state was saved with {len(state.get('altitude_mirrors', ()))} altitude mirrors, this env has {len(self._mirrors)}")
        if self._altitudes is not None:
            # (ranges are fixed at construction: a state taken with others belongs to another geometry)
            far = np.full(self.num_envs, np.inf)
            for what, have, saved in [("source_range", self.source_range, state.get("source_range", far))] + [
                    (f"sightline {name!r}: range", sl.range, state["sightlines"][name].get("range", far)) for name, sl in self._sightlines.items()]:
                if not np.array_equal(np.asarray(saved, dtype=np.float64), have):
                    raise ValueError(f"set_state: the state was saved with {what} = {np.asarray(saved).tolist()}, this env was built with {have.tolist()}")
            # (every angle is checked against this env's margins before anything changes)
            moved = [(self, self._shifts_for(state["field_angle"], "set_state: field_angle", self.source_range))]
            moved += [(sl, self._shifts_for(state["sightlines"][name]["angle"], f"set_state: sightline {name!r}", sl.range))
                      for name, sl in self._sightlines.items()]
            for target, look in moved:
                target._look(*look)
        for lay, st in zip(self._layers, state["layers"]):
            lay.set_state(st)
        for name, sl in self._sightlines.items():
            sl.env.set_state(state["sightlines"][name]["env"])
            sl.last = None
        if self.disturbance is not None:
            self.disturbance.load_state_dict(state["disturbance"])
            self._coeff = self.disturbance.coefficients()
        for m, blob in zip(self._mirrors, state.get("altitude_mirrors", ())):
            m.set_state(blob)
        super().set_state(state)
        self._filter()   # (chi and the diffracted phases are functions of the layers' screens: nothing of them is in the state)
        self._install()   # (the front's blob holds the same tiles; installing again keeps one path)

    def close(self):
        for lay in self.__dict__.get("_layers", ()):
            lay.close()
        self._layers = []
        for sl in self.__dict__.get("_sightlines", {}).values():
            sl.env.close()
        self._sightlines = {}
        for m in self.__dict__.get("_mirrors", ()):
            m.close()
        self._mirrors = []
        if self.__dict__.get("scintillation") is not None:
            self.scintillation.close()
            self.scintillation = None
        if self.__dict__.get("disturbance") is not None:
            self.disturbance.close()
            self.disturbance = None
        super().close()
