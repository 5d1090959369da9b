"""Host restatement of ``aog_install_layer_sum`` (include/aogym.h) in numpy float64, written from the header's definition: the sum of
the layers' ring-buffer screens through each layer's own origin, the removal of the aperture mean, the scaling to revolutions of the
sensing wavelength and the MFMA accumulator order of the fp32 screen tiles.  The only freedom the device has against it is the order
of the float64 additions of the mean: at most n_ap * 2^-53 * max|s| on every value."""
import numpy as np


def tile_index(env, p, n_ptiles):
    """Index of (env, packed aperture pixel p) in the screen tiles: [env / 32][p / 32][g = (p % 32) / 8][lane = 32 h + env % 32][r = p % 4],
    h = ((p % 32) / 4) & 1 (arrays broadcast)."""
    env, p = np.asarray(env), np.asarray(p)
    et, e, pt, i = env >> 5, env & 31, p >> 5, p & 31
    g, h, r = i >> 3, (i >> 2) & 1, i & 3
    return ((((et * n_ptiles + pt) * 4 + g) * 64) + (h * 32 + e)) * 4 + r


def layer_sum(masters, origins, ap_index, N):
    """s [B, n_ap] = sum over l, in layer order, of master_l[b][(iy + oy_l[b]) mod N][(ix + ox_l[b]) mod N] at the aperture pixels
    (iy, ix) = divmod(ap_index, N).  masters: L arrays [B, N, N] (the physical rings); origins: L integer arrays [B, 2] = (ox, oy)."""
    iy, ix = np.divmod(np.asarray(ap_index, dtype=np.int64), N)
    s = None
    for m, o in zip(masters, origins):
        m, o = np.asarray(m, dtype=np.float64), np.asarray(o, dtype=np.int64)
        b = np.arange(m.shape[0])[:, None]
        v = m[b, (iy[None, :] + o[:, 1:2]) % N, (ix[None, :] + o[:, 0:1]) % N]
        s = v if s is None else s + v
    return s


def install(masters, origins, ap_index, N, wavelength_wfs):
    """What the call leaves in a front handle of B envs: dict(s, mean [B], psi64 [B, n_ap] = s - mean (float64 handles), rev [B, n_ap]
    float32 = float((s - mean) / (2 pi lambda_wfs)), tiles float32 [Bp / 32 * n_ptiles * 1024] = rev in accumulator order, zero in
    the padding)."""
    s = layer_sum(masters, origins, ap_index, N)
    B, n_ap = s.shape
    mean = s.sum(axis=1) / n_ap
    psi64 = s - mean[:, None]
    rev = (psi64 * (1.0 / (2.0 * np.pi * wavelength_wfs))).astype(np.float32)
    n_ptiles = (n_ap + 31) // 32
    Bp = (B + 63) // 64 * 64
    tiles = np.zeros(Bp // 32 * n_ptiles * 1024, dtype=np.float32)
    tiles[tile_index(np.arange(B)[:, None], np.arange(n_ap)[None, :], n_ptiles)] = rev
    return dict(s=s, mean=mean, psi64=psi64, rev=rev, tiles=tiles)


def unpack_tiles(tiles, B, n_ap):
    """(rev [B, n_ap], number of nonzero pad entries) of a tile array."""
    tiles = np.asarray(tiles)
    n_ptiles = (n_ap + 31) // 32
    idx = tile_index(np.arange(B)[:, None], np.arange(n_ap)[None, :], n_ptiles)
    pad = np.ones(tiles.shape, dtype=bool)
    pad[idx.ravel()] = False
    return tiles[idx], int(np.count_nonzero(tiles[pad]))


def front_store(env, fp64=False):
    """The front handle's stored screens read back raw out of its state blob (aog_get_state: actuators [B][A] float64, t_render [B] int32,
    screen counters [B] uint32, then the screens, each part padded to 256 bytes): the float32 tiles, or [B, n_ap] float64 on a float64
    handle (``fp64``).  ``env``: a quasi-static env (the front of a LayeredAOEnv)."""
    from adaptive_optics_gym_amd import BatchedAOEnv

    blob = BatchedAOEnv.get_state(env)["blob"].cpu().numpy()
    B, A, n_ap = env.num_envs, env.num_modes, int(env.tables.n_ap)
    r256 = lambda n: (n + 255) // 256 * 256
    off = r256(8 * B * A) + 2 * r256(4 * B)
    if fp64:
        return blob[off:off + 8 * B * n_ap].view(np.float64).reshape(B, n_ap).copy()
    n = (B + 63) // 64 * 2 * ((n_ap + 31) // 32) * 1024
    return blob[off:off + 4 * n].view(np.float32).copy()
