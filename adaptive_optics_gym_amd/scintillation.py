"""Scintillation: weak-turbulence (Rytov) propagation of the layers above the ground to the pupil.

Geometric optics adds a layer's phase to the pupil as if it lay on the aperture.  Over a distance z a phase screen phi diffracts: in the
Fourier domain, with spatial frequency f (cycles per metre),

    S   = F^-1[cos(pi lambda z f^2) F phi]      the phase that arrives
    chi = F^-1[sin(pi lambda z f^2) F phi]      the log-amplitude that arrives

(``kappa^2 z / 2k`` with kappa = 2 pi f and k = 2 pi / lambda is ``pi lambda z f^2``).  A sinusoid of period p keeps its shape and is
split ``cos(pi lambda z / p^2)`` to ``sin(pi lambda z / p^2)`` between the two — the Talbot effect.  The filter is shift-invariant: it runs
once per layer on the meta-pupil (``aog_scint_filter``, ``include/aogym_scintillation.h``) and every front reads the results at its own
shift, as it reads the layer.  Valid for weak scintillation: ``rytov_variance`` gives the theoretical log-amplitude variance of a
profile, and sigma_chi^2 <~ 0.3 is the regime; above it the irradiance saturates, which a first-order filter does not know.

Edges.  The transform runs on the even (mirror) extension of the meta-pupil, which is continuous across the edges, and the meta-pupil
carries a guard band of ``default_guard`` pixels beyond the margin the sightlines need.  Content at spatial frequency f reaches
``lambda z f`` sideways, so what lies beyond the guard is missing from the footprint's scales finer than ``guard x pitch / (lambda z)``
(mirrored screen stands in for it: the statistics hold, the detail does not); the error only stops falling at a guard of
``lambda z / (2 pitch)``, the reach of the pixel Nyquist frequency, which no batch can afford.  ``profiles/scintillation.md`` has the
measured error against the guard and says what the default buys.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from .atmosphere_host import _R0_UNIT, cn_squared_from_fried_parameter
from .device_handle import DeviceHandle, ptr

MAX_FIBER = _lib.SCINT_MAX_FIBER
GUARD_ZONES = 2.0               # the default guard band in Fresnel zones of the highest layer (profiles/scintillation.md)
REGIME = 0.3                    # the log-amplitude variance below which the Rytov filter is trusted
SCRATCH_BYTES = 256 << 20       # the transform buffer's default byte budget (it does not grow with the batch)


def default_guard(altitudes, wavelength, pitch):
    """The default guard band in pixels: ``GUARD_ZONES`` Fresnel zones sqrt(lambda h) of the highest layer, rounded up (0 when every
    layer is on the ground)."""
    h = float(np.max(np.asarray(altitudes, dtype=np.float64), initial=0.0))
    return int(math.ceil(GUARD_ZONES * math.sqrt(wavelength * h) / pitch)) if h > 0 else 0


def resolve_scintillation(spec):
    """``scintillation=`` checked: None / False (off), True (defaults) or a dict with 'guard' (pixels, an integer >= 0; None: the default)
    and 'scratch_bytes' (> 0).  Returns None or dict(guard=, scratch_bytes=).  ``ValueError`` otherwise."""
    if spec is None or spec is False:
        return None
    if spec is True:
        spec = {}
    if not isinstance(spec, dict) or not set(spec) <= {"guard", "scratch_bytes"}:
        raise ValueError("scintillation: True, or a dict with 'guard' and / or 'scratch_bytes'")
    guard = spec.get("guard")
    if guard is not None and (int(guard) != guard or guard < 0):
        raise ValueError(f"scintillation: guard is a number of pixels, an integer >= 0, got {guard!r}")
    scratch = spec.get("scratch_bytes", SCRATCH_BYTES)
    if int(scratch) != scratch or scratch < 1:
        raise ValueError(f"scintillation: scratch_bytes must be a positive integer, got {scratch!r}")
    return dict(guard=None if guard is None else int(guard), scratch_bytes=int(scratch))


def _frequencies_squared(shape, pitch, guard):
    """f^2 (cycles per metre, squared) on the FFT grid of the mirror extension: E = 2 (shape + 2 guard) points per axis."""
    ey, ex = (2 * (int(n) + 2 * int(guard)) for n in shape)
    fy, fx = np.fft.fftfreq(ey, pitch), np.fft.fftfreq(ex, pitch)
    return fy[:, None] ** 2 + fx[None, :] ** 2


def rytov_filters(altitudes, wavelength, pitch, shape, guard=0):
    """The host table of the filter: [L, Ey, Ex, 2] float64 (cos, sin) of ``pi lambda h_l f^2`` at the FFT frequencies of the mirror
    extension of a meta-pupil of ``shape`` = (My, Mx) pixels plus ``guard`` pixels on every side (Ey = 2 (My + 2 guard)).  The device
    multiplies by this very table (it evaluates no transcendental) and so does the host restatement.  A layer at h = 0 gets (1, 0)."""
    h = np.asarray(altitudes, dtype=np.float64)
    if h.ndim != 1 or not np.all(np.isfinite(h)) or np.any(h < 0):
        raise ValueError("rytov_filters: altitudes are finite and >= 0, one per layer")
    arg = (math.pi * float(wavelength)) * h[:, None, None] * _frequencies_squared(shape, pitch, guard)[None]
    return np.ascontiguousarray(np.stack([np.cos(arg), np.sin(arg)], axis=-1))


def rytov_variance(altitudes, fractions, fried, wavelength, pitch, shape, guard=0, outer_scale=10.0, fried_wavelength=None):
    """The theoretical log-amplitude variance sigma_chi^2 (nepers^2) of a profile: the project's von Karman spectrum
    (``atmosphere_host.spectral_amplitude``'s PSD, Cn^2 of layer l = fraction_l x Cn^2(r0)) integrated against sin^2(pi lambda h_l f^2) on
    the discrete frequency grid of ``rytov_filters``.  ``fried``: a scalar or per-env values, the r0 at ``fried_wavelength`` (default:
    ``wavelength``; the envs state their r0 at the science wavelength); returns a float or an array like it.
    sigma_chi^2 <~ 0.3 (``REGIME``) is where the first-order filter holds."""
    h = np.asarray(altitudes, dtype=np.float64)
    w = np.asarray(fractions, dtype=np.float64)
    f2 = _frequencies_squared(shape, pitch, guard)
    ey, ex = f2.shape
    du2 = (2 * math.pi / (ey * pitch)) * (2 * math.pi / (ex * pitch))
    u2, u0 = (2 * math.pi) ** 2 * f2, 2 * math.pi / outer_scale
    psd = 0.0229 * _R0_UNIT ** (-5.0 / 3.0) * ((u2 + u0 * u0) / (2 * math.pi) ** 2) ** (-11.0 / 6.0)
    psd[f2 == 0] = 0.0
    cell = psd * du2 / (2 * math.pi) ** 2      # the variance of a unit-Cn^2 screen (phase x lambda) per frequency cell
    unit = sum(wl * float(np.sum(np.sin(math.pi * wavelength * hl * f2) ** 2 * cell)) for hl, wl in zip(h, w))
    at = wavelength if fried_wavelength is None else fried_wavelength
    cn2 = np.asarray([cn_squared_from_fried_parameter(r, at) for r in np.atleast_1d(np.asarray(fried, dtype=np.float64))])
    out = unit * cn2 / wavelength ** 2
    return float(out[0]) if np.ndim(fried) == 0 else out


def receive_modes(tables):
    """[n_fiber, n_ap] complex: the fibre's modes folded to the pupil, whose overlaps with the field the step's power sums
    (``optics_host.build_tables``: the last ``n_fiber_modes`` rows of ``wfs_coef @ wfs_tables``)."""
    k = int(tables.n_fiber_modes)
    return np.ascontiguousarray(tables.wfs_coef[-k:] @ tables.wfs_tables)


class _Correction:
    """A layer's diffraction correction S - phi as ``install_layer_sum_conjugate`` takes a mirror: a handle the ``Scintillation`` owns."""

    def __init__(self, address):
        self._handle = C.c_void_p(address)


class Scintillation(DeviceHandle):
    """The device object (``aog_scint_*``): the filter tables of the layers above the ground and, per such layer, the float64 meta-pupil
    surfaces S - phi and chi.

    env        a ``LayeredAOEnv`` built with ``layer_altitudes`` (its meta-pupil is the filter's grid, guard band included)
    layers     the indices of the layers above the ground, in layer order (none: a receiver only)

    ``filter()`` runs after the layers evolved; ``corrections`` are what the installation reads beside the layers; ``install(front, ...)``
    writes a front's float32 log-amplitude map in the screen tiles' order and ``receive(front, chi_tile)`` returns the receiver's dict.
    There is no state: chi is a function of the layers' screens."""

    prefix, noun = "aog_scint", "scintillation"

    def __init__(self, env, layers, scratch_bytes=SCRATCH_BYTES):
        import torch

        self._layers = [env.layers[i] for i in layers]
        self.layer_index = list(layers)
        self.n_pixels = int(env.meta_pupil_pixels)
        self.num_envs = int(env.num_envs)
        modes = receive_modes(env.tables)
        if modes.shape[0] > MAX_FIBER:
            raise ValueError(f"scintillation: the receiver holds at most {MAX_FIBER} fibre modes, these tables have {modes.shape[0]}")
        self.n_fiber = int(modes.shape[0])
        self._scratch = int(scratch_bytes)
        self._bind(torch, env.device, self.num_envs)
        self._create()
        self.table = rytov_filters(env.layer_altitudes[self.layer_index], env.params.wavelength_wfs, env.params.pupil_pixel, (self.n_pixels,) * 2, 0)
        if self._layers:
            t = torch.from_numpy(self.table).to(self.device)
            self._call("upload", ptr(t), self._stream())
            torch.cuda.current_stream(self.device).synchronize()   # (t is a temporary)
        packed = np.ascontiguousarray(np.stack([modes.real, modes.imag], axis=-1), dtype=np.float64)
        self._call("upload_modes", env._handle, C.c_void_p(packed.ctypes.data))
        self.corrections = [_Correction(self.lib.aog_scint_correction(self._handle, l)) for l in range(len(self._layers))]
        self._handles = (C.c_void_p * max(1, len(self._layers)))(*[lay._handle.value for lay in self._layers])

    def _config(self):
        return _lib.AogScintConfig(_lib.ABI_VERSION, self.num_envs, self.n_pixels, len(self._layers), self.n_fiber, 0, self._scratch)

    scratch_bytes = property(lambda self: int(self.lib.aog_scint_scratch_bytes(self._handle)),
                             doc="bytes of the transform buffer and hipFFT's work area: bounded by the budget, whatever the batch")

    def filter(self):
        """S - phi and chi of every layer above the ground from the layers' current screens (``aog_scint_filter``), on the current stream."""
        self._call("filter", self._handles, self._stream())

    def surfaces(self, layer):
        """(S - phi, chi) of filtered layer ``layer`` (an index into ``layer_index``): two [B, M, M] float64 tensors, in the masters' unit."""
        torch = self._torch
        out = [torch.empty((self.num_envs, self.n_pixels, self.n_pixels), dtype=torch.float64, device=self.device) for _ in range(2)]
        self._call("get", int(layer), ptr(out[0]), ptr(out[1]), self._stream())
        return tuple(out)

    def tile(self, front):
        """A zeroed float32 log-amplitude map for ``front`` (a fast ``BatchedAOEnv``), in its screen tiles' packed order."""
        n = int(self.lib.aog_scint_tile_floats(front._handle))
        return self._torch.zeros((n,), dtype=self._torch.float32, device=self.device)

    def install(self, front, shifts, shifts_dev, chi_tile):
        """``chi_tile`` = the sum of the chi surfaces at ``shifts`` ([L', B, 2] float64 host array of the filtered layers' shifts;
        ``shifts_dev`` the same on the device) in nepers (``aog_scint_install``)."""
        self._call("install", front._handle, C.c_void_p(shifts.ctypes.data), ptr(shifts_dev), ptr(chi_tile), self._stream())

    def receive(self, front, chi_tile):
        """dict(power, irradiance, strehl, sigma_chi2) of [B] float64 device tensors (``aog_scint_receive``); ``chi_tile`` None: chi = 0."""
        torch = self._torch
        out = {k: torch.empty((self.num_envs,), dtype=torch.float64, device=self.device) for k in ("power", "irradiance", "strehl", "sigma_chi2")}
        self._call("receive", front._handle, ptr(chi_tile), *(ptr(out[k]) for k in ("power", "irradiance", "strehl", "sigma_chi2")), self._stream())
        return out

    def unpack_tile(self, front, chi_tile, first=0, count=None):
        """[count, N, N] float32: a log-amplitude map on the pupil grid (zeros outside the aperture)."""
        torch = self._torch
        B, N, n_ap = self.num_envs, front.num_pupil_pixels, int(front.tables.n_ap)
        count = B - first if count is None else int(count)
        env = torch.arange(first, first + count, device=self.device)[:, None]
        p = torch.arange(n_ap, device=self.device)[None, :]
        n_ptiles = int(front.info.n_ap_padded) // 32
        i = p & 31
        index = ((((env >> 5) * n_ptiles + (p >> 5)) * 4 + (i >> 3)) * 64 + (((i >> 2) & 1) * 32 + (env & 31))) * 4 + (i & 3)
        out = torch.zeros((count, N * N), dtype=torch.float32, device=self.device)
        out[:, torch.from_numpy(np.asarray(front.tables.ap_index, dtype=np.int64)).to(self.device)] = chi_tile[index]
        return out.view(count, N, N)

    def get_state(self):
        """Nothing: chi is a function of the layers' screens (a resumed env filters again)."""
        return None

    def set_state(self, blob):
        if blob is not None:
            raise ValueError("set_state: a scintillation has no state")
