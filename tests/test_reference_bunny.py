"""The PLY loader on the reference's own data/tests/bunny.ply (stored whole,
xz-compressed, as tests/golden/bunny.ply.xz; conftest.reference_bunny_path unpacks
it), and C3 (matpreview) with the bunny as its object rendered by the CPU
oracle.  The benchmark's C3 keeps the procedural stand-in (scenes.blob_mesh)."""
import numpy as np

from conftest import reference_bunny_path
from mitsuba_amd import ply, scenes
from mitsuba_amd.transform import Transform

BUNNY = reference_bunny_path()


def _bunny_world():
    """bunny.ply scaled to 2 units tall, standing on y = 0 at the origin (matpreview's object slot)."""
    m0 = ply.load_ply(BUNNY)
    lo, hi = m0.positions.min(0), m0.positions.max(0)
    s = 2.0 / float(hi[1] - lo[1])
    c = 0.5 * (lo + hi)
    to_world = Transform().translate(-float(c[0]), -float(lo[1]), -float(c[2])).scale(s)   # scale after centring
    return ply.load_ply(BUNNY, toWorld=to_world, name='bunny')


def test_bunny_ply_loads():
    m = ply.load_ply(BUNNY)
    assert m.positions.shape == (35947, 3) and m.indices.shape == (69451, 3)   # 69,451 tris
    assert m.indices.max() < m.positions.shape[0] and np.isfinite(m.positions).all()
    w = _bunny_world()
    lo, hi = w.positions.min(0), w.positions.max(0)
    np.testing.assert_allclose([lo[1], hi[1]], [0.0, 2.0], atol=1e-5)


def test_matpreview_on_the_bunny_renders(oracle):
    sc, it = scenes.build('C3', width=48, height=32, spp=4, env_size=(64, 32), object_mesh=_bunny_world())
    assert sc.meshes[0].name == 'bunny' and sc.num_triangles >= 69451
    film, _, st = oracle.render(sc, it, libm_mode=0)
    rgb = film[..., :3]
    assert np.isfinite(rgb).all() and rgb.min() >= 0 and rgb.max() > 0
    assert st['samples'] == 48 * 32 * 4
    # the bunny is in view: the frame differs from the same scene without it
    sc2, _ = scenes.build('C3', width=48, height=32, spp=4, env_size=(64, 32), blob=(8, 6))
    film2, _, _ = oracle.render(sc2, it, libm_mode=0)
    assert np.abs(film2[..., :3] - rgb).max() > 1e-3
