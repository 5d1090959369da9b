"""Every instantiation the layer-sum installation dispatches to: the three forms (plain, disturbed, sightline) at every layer count
L = 1 .. 8, bit for bit against the host restatements of the neighbouring suites (layered_reference, disturbance_reference,
sightline_reference).  Those suites stop at L = 3; the dispatch over L and the form is one piece of code, and this module walks all of it.

N = 32, B = 33: two env tiles, the second with 31 pad envs, and 25 pixel tiles, so the last workgroup of the tile pass leaves its loop
early.  The sightline form reads layers of N_L = 48 (margin 8) at random fractional shifts inside the margin.  K = 2 where terms apply."""
import numpy as np
import pytest

import disturbance_reference as dref
import layered_reference as lref
import sightline_reference as sref
from test_gpu_disturbance import _static_env, _upload
from test_gpu_layered import _kw
from test_gpu_parity import _torch
from test_gpu_sightline import MARGIN, N, NL, _meta_params

pytestmark = pytest.mark.gpu

B, K = 33, 2
FORMS = ("plain", "disturbed", "sightline")


@pytest.fixture(scope="module")
def layers8():
    """{N_l: eight evolved dynamic layers of N_l pixels} (shared by every case; nothing below changes them), with their screens on the host."""
    torch = _torch()
    from adaptive_optics_gym_amd import BatchedAOEnv

    sets = {}
    for n in (N, NL):
        lays = [BatchedAOEnv(B, "cuda:0", atm_type="dynamic", atm_vel=30.0 + 10.0 * i, atm_fried=0.15, seed=3 + i, params=_meta_params(n), **_kw(N=n, T=0))
                for i in range(8)]
        for lay in lays:
            for _ in range(3):
                lay.evolve_atmosphere()
        sets[n] = (lays, [lay.get_screens().cpu().numpy() for lay in lays])
    torch.cuda.synchronize()
    yield sets
    for lays, _ in sets.values():
        for lay in lays:
            lay.close()


def _check(layers8, form, L, precision):
    torch = _torch()
    from adaptive_optics_gym_amd.layered import LayeredAOEnv, install_layer_sum_sightline

    lays, screens = layers8[NL if form == "sightline" else N]
    lays, screens = lays[:L], screens[:L]
    front = _static_env(B, N=N, precision=precision)
    try:
        ap = np.asarray(front.tables.ap_index)
        n_ap = ap.size
        assert n_ap % 64 != 0
        rng = np.random.RandomState(1000 * FORMS.index(form) + L)
        basis = coeff = cdev = None
        if form != "plain":
            basis, coeff = rng.randn(K, n_ap) * 2 * np.pi, rng.randn(B, K) * 1e-7
            assert _upload(front, basis)[0] == 0
            cdev = torch.from_numpy(coeff).cuda()
        zero = [np.zeros((B, 2), dtype=int)] * L      # (get_screens() is logical: the ring origins are already undone)
        if form == "plain":
            front.install_layer_sum(lays)
            want = dref.install(screens, zero, ap, N, front.wavelength_wfs, np.zeros((B, 0)), np.zeros((0, n_ap)))   # (no terms; the mean in the fixed order)
        elif form == "disturbed":
            LayeredAOEnv.install_layer_sum_disturbed(front, lays, cdev)      # (the env's own wrapper on a bare front: it needs nothing else of the env)
            want = dref.install(screens, zero, ap, N, front.wavelength_wfs, coeff, basis)
        else:
            shifts = rng.uniform(-(MARGIN - 1), MARGIN - 1, size=(L, B, 2))
            assert (shifts != np.floor(shifts)).all()
            install_layer_sum_sightline(front, lays, shifts, cdev)
            want = sref.install(screens, shifts, ap, N, front.wavelength_wfs, coeff, basis)
        fp64 = precision == "fp64"
        got = lref.front_store(front, fp64=fp64)
        ref = want["psi64"] if fp64 else want["tiles"]
        assert got.shape == ref.shape and np.abs(got).max() > 0
        print(f"{form} L={L} {precision}: {np.count_nonzero(got != ref)} of {got.size} values differ")
        np.testing.assert_array_equal(got, ref)
    finally:
        front.close()


@pytest.mark.parametrize("L", range(1, 9))
@pytest.mark.parametrize("form", FORMS)
def test_every_layer_count_of_every_form_on_a_fast_front(layers8, form, L):
    _check(layers8, form, L, "fast")


@pytest.mark.parametrize("L", [2, 8])
@pytest.mark.parametrize("form", FORMS)
def test_the_float64_front_at_two_layer_counts(layers8, form, L):
    _check(layers8, form, L, "fp64")
