"""The reprojection rule of DESIGN.md 16 on the CPU (tests/reproject_ref.py, visibility from the oracle's closest-hit query):
the projection inverts ray generation, an unmoved view is an exact copy, a whole-pixel camera shift is the shifted copy, and a
moved instance disoccludes what it uncovers.  tests/test_gpu_reproject.py holds the device to the same restatement."""
import numpy as np
import pytest

from lupinpathtracer_amd import api, loader
from tests import reproject_ref as R
from tests import util


def _rot(ax, ay, az):
    def r(a, i, j):
        m = np.eye(3)
        m[i, i] = m[j, j] = np.cos(a)
        m[i, j], m[j, i] = -np.sin(a), np.sin(a)
        return m
    return r(ax, 1, 2) @ r(ay, 2, 0) @ r(az, 0, 1)


def _transform(rot, pos):
    """(4, 3): three columns of the rotation, then the translation."""
    return np.concatenate([np.asarray(rot, np.float64).T, np.asarray(pos, np.float64)[None]], 0).astype(np.float32)


CAMERAS = [
    ("identity", np.eye(3), (0.0, 0.0, 0.0)),
    ("translated", np.eye(3), (1.5, -0.75, -3.0)),
    ("rotated", _rot(0.3, -0.7, 0.2), (0.0, 0.0, 0.0)),
    ("rotated_translated", _rot(-1.1, 2.4, 0.6), (-2.0, 1.0, 3.0)),
]


@pytest.mark.parametrize("cam_name,rot,pos", CAMERAS, ids=[c[0] for c in CAMERAS])
@pytest.mark.parametrize("aspect", [16.0 / 9.0, 0.75])
@pytest.mark.parametrize("ortho", [False, True], ids=["perspective", "orthographic"])
def test_projection_inverts_ray_generation(built, ortho, aspect, cam_name, rot, pos):
    """A point along the restated centre ray of pixel (gx, gy) projects to (gx, gy) within 1/128 pixel -- half the snap step, so
    the snap of an unmoved view lands on the pixel centre -- at 3840 x 2160.  The round trip goes through f32 world
    coordinates, so its error is a few ulp of |world| seen from the point's distance: the cameras sit within a few units of the
    origin and the points 2 to 10 units in front of them, the proportions of the fixture scenes."""
    W, H = 3840, 2160
    cp = api.CameraParams(is_orthographic=ortho, lens=0.05, film=0.036, aspect=aspect, focus=5.0, aperture=0.0)
    tr = _transform(rot, pos)
    ori, d = R.centre_rays(W, H, cp, tr)
    rng = np.random.default_rng(7)
    ys = np.concatenate([[0, 0, H - 1, H - 1, H // 2], rng.integers(0, H, 4000)])
    xs = np.concatenate([[0, W - 1, 0, W - 1, W // 2], rng.integers(0, W, 4000)])
    t = np.concatenate([[2.0] * 5, rng.uniform(2.0, 10.0, 4000)]).astype(np.float32)
    p = ori[ys, xs] + d[ys, xs] * t[:, None]
    pc = R.mat_point(R.camera_inverse(tr), p)
    assert (pc[:, 2] > 0).all()
    fx, fy = R.project(cp, W, H, pc)
    ex, ey = np.abs(fx - xs).max(), np.abs(fy - ys).max()
    print(f"{cam_name} ortho={ortho} aspect={aspect:.3f}: max |fx - gx| {ex:.2e}, max |fy - gy| {ey:.2e} pixel")
    assert ex <= 1.0 / 128 and ey <= 1.0 / 128


def _random_state(H, W, seed, nmax=9):
    rng = np.random.default_rng(seed)
    frames = rng.integers(1, nmax + 1, (H, W)).astype(np.uint32)
    moments = np.stack([rng.uniform(0.0, 2.0, (H, W)), rng.uniform(0.0, 5.0, (H, W))], -1).astype(np.float32)
    texel = np.ones((H, W, 4), np.float16)
    texel[..., :3] = rng.uniform(0.0, 4.0, (H, W, 3)).astype(np.float16)
    return frames, moments, texel


def test_identity_copies_texel_count_and_moments(built):
    scene, cams = util.load_scene("cornellbox_builtin")
    cam, W, H = cams[0], 64, 48
    cp = api.CameraParams(**{**cam.params.__dict__, "aspect": W / H})
    vis = R.visibility_from_oracle(scene, W, H, cp, cam.transform)
    hit = vis[0] != R.MISS
    assert hit.mean() > 0.9
    frames, moments, texel = _random_state(H, W, 1)
    tris, _ = R.scene_triangles(scene)
    rows = R.local_to_world_rows(scene.instances["transpose_inverse_transform"])
    col, out, n, mom = R.gather(vis, vis, cp, cam.transform, tris, rows, frames, moments, texel[..., :3].astype(np.float32), 0.02)
    assert np.array_equal(out.view(np.uint16)[hit], texel.view(np.uint16)[hit])
    assert np.array_equal(n[hit], frames[hit])
    assert np.array_equal(mom.view(np.uint32)[hit], moments.view(np.uint32)[hit])
    assert (n[~hit] == 0).all() and (mom[~hit] == 0).all() and (out[~hit] == np.array([0, 0, 0, 1], np.float16)).all()
    # a cap lowers the counts and rescales M2, nothing else
    col2, out2, n2, mom2 = R.gather(vis, vis, cp, cam.transform, tris, rows, frames, moments, texel[..., :3].astype(np.float32), 0.02, max_history=2)
    assert np.array_equal(n2[hit], np.minimum(frames, 2)[hit]) and np.array_equal(out2, out)
    assert np.array_equal(mom2[..., 0], mom[..., 0])
    want = np.where(frames <= 2, moments[..., 1], (moments[..., 1] / frames.astype(np.float32)) * np.minimum(frames, 2).astype(np.float32))
    assert np.array_equal(mom2[..., 1][hit], want.astype(np.float32)[hit])
    # without a previous view nothing survives
    _, out3, n3, mom3 = R.gather(vis, vis, cp, cam.transform, tris, rows, frames, moments, texel[..., :3].astype(np.float32), 0.02, prev_valid=False)
    assert (n3 == 0).all() and (mom3 == 0).all() and (out3 == np.array([0, 0, 0, 1], np.float16)).all()


def _plane_visibility(W, H, cp, tr, tri, z_plane):
    """Visibility of one big triangle in the plane z = z_plane seen by an axis-aligned orthographic camera: barycentrics
    solved in float64 from the centre rays."""
    ori, d = R.centre_rays(W, H, cp, tr)
    assert np.array_equal(d.reshape(-1, 3), np.tile(np.array([0, 0, 1], np.float32), (W * H, 1)))
    t = (np.float32(z_plane) - ori[..., 2]).astype(np.float32)
    p = ori.astype(np.float64) + d.astype(np.float64) * t[..., None]
    a, b, c = tri.astype(np.float64)
    m = np.stack([b - a, c - a], -1)[:2]   # the triangle lies in a z plane: solve in x, y
    uv = np.linalg.solve(m, (p[..., :2] - a[:2]).reshape(-1, 2).T).T.reshape(H, W, 2)
    assert (uv >= 0).all() and (uv.sum(-1) <= 1).all()
    return (np.zeros((H, W), np.uint32), np.zeros((H, W), np.uint32), uv.astype(np.float32), R.depth_of(tr, ori, d, t))


@pytest.mark.parametrize("shift", [3, -5])
def test_whole_pixel_shift_of_an_orthographic_camera(built, shift):
    """Translating the camera by k pixels along +x makes new pixel gx show what pixel gx + k showed; the strip that was outside
    the old view has no history."""
    W, H = 40, 24
    cp = api.CameraParams(is_orthographic=True, lens=0.05, film=0.036, aspect=W / H, focus=10.0, aperture=0.0)
    pixel = 0.036 / 0.05 / W   # world size of a pixel: fsx / lens / W
    tri = np.array([[-4, -4, 2], [8, -4, 2], [-4, 8, 2]], np.float32)
    old = _transform(np.eye(3), (0.0, 0.0, 0.0))
    new = _transform(np.eye(3), (shift * pixel, 0.0, 0.0))
    prev, cur = _plane_visibility(W, H, cp, old, tri, 2.0), _plane_visibility(W, H, cp, new, tri, 2.0)
    frames, moments, texel = _random_state(H, W, 2)
    rows = R.local_to_world_rows(np.eye(3, 4, dtype=np.float32)[None])
    _, out, n, mom = R.gather(cur, prev, cp, old, tri[None], rows, frames, moments, texel[..., :3].astype(np.float32), 0.02)
    src = np.arange(W) + shift
    inside = (src >= 0) & (src < W)
    assert np.array_equal(out[:, inside].view(np.uint16), texel[:, src[inside]].view(np.uint16))
    assert np.array_equal(n[:, inside], frames[:, src[inside]])
    assert np.array_equal(mom[:, inside].view(np.uint32), moments[:, src[inside]].view(np.uint32))
    assert inside.sum() == W - abs(shift)
    assert (n[:, ~inside] == 0).all() and (mom[:, ~inside] == 0).all()
    assert (out[:, ~inside] == np.array([0, 0, 0, 1], np.float16)).all()


def test_a_moved_instance_disoccludes(built):
    """Every pixel whose instance differs from the instance the previous view saw at its reprojected location starts afresh."""
    W, H = 64, 48
    scene_cpu, cams = loader.cornell_box_scene_cpu()
    cam = cams[0]
    cp = api.CameraParams(**{**cam.params.__dict__, "aspect": W / H})
    old_scene = api.build_accel_structures_and_upload(None, scene_cpu, [], [], True)
    moved = 5   # the short box
    new_cpu, _ = loader.cornell_box_scene_cpu()
    l2w = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-0.35, 0.0, 0.1]], np.float32)
    new_cpu.instances[moved] = api.instance_from_transform(l2w, moved, int(new_cpu.instances[moved]["mat_idx"]))
    new_scene = api.build_accel_structures_and_upload(None, new_cpu, [], [], True)
    prev = R.visibility_from_oracle(old_scene, W, H, cp, cam.transform)
    cur = R.visibility_from_oracle(new_scene, W, H, cp, cam.transform)
    frames, moments, texel = _random_state(H, W, 3)
    tris, _ = R.scene_triangles(new_scene)
    rows = R.local_to_world_rows(old_scene.instances["transpose_inverse_transform"])
    _, out, n, mom = R.gather(cur, prev, cp, cam.transform, tris, rows, frames, moments, texel[..., :3].astype(np.float32), 0.02)
    hit = cur[0] != R.MISS
    # where the hit point was in the previous view, computed apart from the gather (float64, nearest pixel)
    idx = np.nonzero(hit.reshape(-1))[0]
    tv = tris[cur[1].reshape(-1)[idx]].astype(np.float64)
    u, v = cur[2].reshape(-1, 2)[idx].astype(np.float64).T
    pl = tv[:, 0] * (1 - u - v)[:, None] + tv[:, 1] * u[:, None] + tv[:, 2] * v[:, None]
    r = rows[cur[0].reshape(-1)[idx]].astype(np.float64)
    pw = np.einsum("nkc,nc->nk", r[:, :, :3], pl) + r[:, :, 3]
    fx, fy = R.project(cp, W, H, R.mat_point(R.camera_inverse(cam.transform), pw.astype(np.float32)))
    qx, qy = np.rint(fx).astype(int), np.rint(fy).astype(int)
    on_centre = (np.abs(fx - qx) < 1e-3) & (np.abs(fy - qy) < 1e-3) & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
    seen = np.where(on_centre, prev[0][np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)], R.MISS)
    differs = on_centre & (seen != cur[0].reshape(-1)[idx])
    still = cur[0].reshape(-1)[idx] != moved
    assert differs.sum() > 20, "the move uncovered nothing"
    assert (n.reshape(-1)[idx][differs] == 0).all()
    assert (mom.reshape(-1, 2)[idx][differs] == 0).all()
    # unmoved surfaces that the previous view saw too keep their history, exactly (they land on pixel centres)
    same = on_centre & still & (seen == cur[0].reshape(-1)[idx])
    assert same.sum() > 1000
    assert np.array_equal(n.reshape(-1)[idx][same], frames.reshape(-1)[idx][same])
    # the moved box itself is found again at its old place: history follows the instance
    box = (~still) & (n.reshape(-1)[idx] > 0)
    assert box.sum() > 20
