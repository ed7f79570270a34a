"""CPU: tests/draw_oracle.py against closed forms, the submit wiring of `--postprocess_draw` with stub fitter and drawer, MeshDrawer's host
half with the kernel replaced by the oracle, HO3D.get_obj_faces, and the exemption cap of the GPU test's end-to-end scenes."""
import io
import json
import os
import sys
import warnings

import numpy as np
import pytest
import torch

import draw_oracle as do
import draw_scenes as ds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _raster(pts, faces, W=16, H=16, z=None, ok=None):
    pts = np.asarray(pts, np.float64)
    sx, sy = do.snap(pts[:, 0]), do.snap(pts[:, 1])
    zq = np.asarray(z if z is not None else np.full(len(pts), 1000), np.int64)
    return do.raster_stage(sx, sy, zq, np.ones(len(pts), bool) if ok is None else ok, np.asarray(faces), W, H)


def test_fronto_parallel_square_covers_the_predicted_pixels():
    # corners ON pixel centres.  The project's shared-edge rule (oracle/render_oracle.c: an edge (dx, dy) of the triangle oriented to positive
    # area is inclusive iff dy > 0 or dy == 0 and dx < 0) makes, on the y-down screen, the right and bottom edges inclusive, the left and top not
    k = _raster([[2.5, 3.5], [9.5, 3.5], [9.5, 8.5], [2.5, 8.5]], [[0, 1, 2], [0, 2, 3]])
    want = np.zeros((16, 16), bool)
    want[4:9, 3:10] = True
    assert np.array_equal(k != do.EMPTY, want)
    k = _raster([[2.2, 3.7], [9.9, 3.7], [9.9, 8.1], [2.2, 8.1]], [[0, 1, 2], [0, 2, 3]])
    want[:] = False
    want[4:8, 2:10] = True
    assert np.array_equal(k != do.EMPTY, want)


def test_shared_edges_cover_each_centre_exactly_once():
    rng = np.random.default_rng(0)
    for trial in range(40):
        p = rng.uniform(1, 15, (4, 2))
        if trial % 2:
            p = np.round(p) + 0.5                                  # edges through pixel centres
        # a quad split along p0-p2, either winding; count coverage per triangle
        for f in ([[0, 1, 2], [0, 2, 3]], [[0, 2, 1], [0, 2, 3]]):
            a, b = _raster(p, [f[0]]) != do.EMPTY, _raster(p, [f[1]]) != do.EMPTY
            e = p[2] - p[0]
            d1, d3 = e[0] * (p[1] - p[0])[1] - e[1] * (p[1] - p[0])[0], e[0] * (p[3] - p[0])[1] - e[1] * (p[3] - p[0])[0]
            if d1 * d3 < 0:                                         # p1 and p3 on opposite sides of the shared edge: no overlap allowed
                assert not (a & b).any(), (trial, p)
                both = _raster(p, f) != do.EMPTY
                assert np.array_equal(both, a | b)


def test_nearer_wins_and_ties_go_to_the_lower_index():
    pts = [[1.2, 1.2], [12.2, 1.2], [1.2, 12.2]] * 2
    k = _raster(pts, [[0, 1, 2], [3, 4, 5]], z=[500] * 3 + [400] * 3)
    cov = k != do.EMPTY
    assert cov.any() and ((k[cov] & np.uint64(0xFFFFFFFF)) == 1).all() and ((k[cov] >> np.uint64(32)) == 400).all()
    k = _raster(pts, [[0, 1, 2], [3, 4, 5]], z=[400] * 6)
    assert ((k[cov] & np.uint64(0xFFFFFFFF)) == 0).all()


def test_a_triangle_crossing_the_near_plane_is_dropped_whole():
    K = np.array([[100.0, 0, 8], [0, 100.0, 8], [0, 0, 1]])
    hv = np.zeros((778, 3)); hv[:, 2] = -1.0
    hv[:3] = [[-0.02, -0.02, 0.5], [0.02, -0.02, 0.5], [0.0, 0.02, 0.5]]
    vs = do.vertex_stage(hv, np.array([[0, 1, 2]]), K, 16, 16)
    d = vs[0]
    assert (do.raster_stage(d["sx"], d["sy"], d["zq"], d["ok"], vs["faces"], 16, 16) != do.EMPTY).sum() > 0
    hv[2, 2] = do.NEAR                                              # at the near plane: not in front of it
    vs = do.vertex_stage(hv, np.array([[0, 1, 2]]), K, 16, 16)
    d = vs[0]
    assert not d["ok"][2] and (do.raster_stage(d["sx"], d["sy"], d["zq"], d["ok"], vs["faces"], 16, 16) == do.EMPTY).all()


def test_lambert_closed_form(monkeypatch):
    light = np.array([0.0, 0.0, -10.0])
    monkeypatch.setattr(do, "lights", lambda: (light[None], np.array([0.7])))
    P = np.array([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0]])
    n = np.array([[0.0, 0.0, -2.0], [0.0, 0.0, -1.0]])
    c = do.lambert(P, n, do.HAND_COLOR)
    np.testing.assert_allclose(c[0], do.HAND_COLOR * 0.7, rtol=1e-15)
    np.testing.assert_allclose(c[1], do.HAND_COLOR * 0.7 * 10.0 / np.sqrt(109.0), rtol=1e-15)
    assert (do.lambert(P, -n, do.HAND_COLOR) == 0).all()            # facing away: black


def test_light_positions_are_the_rotated_reference_ones():
    pos, col = do.lights()
    c, s = np.cos(np.radians(120)), np.sin(np.radians(120))
    np.testing.assert_allclose(pos[0], [-200 * c + 100 * s, -100, -200 * s - 100 * c], rtol=1e-12)
    assert list(col) == [1.0, 1.0, 0.7]


def test_orbit_camera_centres_its_look_at_point():
    H = W = 256
    c = np.array([0.03, -0.02, 0.55])
    Rv, pos, focal = do.orbit_camera(c, H)
    np.testing.assert_allclose(Rv @ Rv.T, np.eye(3), atol=1e-14)
    assert np.linalg.det(Rv) > 0
    np.testing.assert_allclose(np.linalg.norm(pos - c), 0.6, rtol=1e-14)
    np.testing.assert_allclose(focal, 128 / np.tan(np.radians(15)), rtol=1e-14)
    pts = np.stack([c, c + [0, 0, 0.1], c - 0.1 * Rv[1]])
    x, y, ok = do.project(focal, focal, W / 2, H / 2, (pts - pos) @ Rv.T)
    assert ok.all()
    np.testing.assert_allclose([x[0], y[0]], [128, 128], atol=1e-10)
    np.testing.assert_allclose(x[1], 128, atol=1e-10)               # the data frame's +z is "up" on the panel
    assert y[1] < 128 - 20
    np.testing.assert_allclose([x[2], y[2]], [128, 128 - focal * 0.1 / 0.6], atol=1e-9)
    # elevation 50 degrees from +z, azimuth -50 degrees from +x towards -y
    u = (pos - c) / 0.6
    np.testing.assert_allclose(np.degrees(np.arccos(u[2])), 50, atol=1e-10)
    np.testing.assert_allclose(np.degrees(np.arctan2(u[1], u[0])), -50, atol=1e-10)


def test_package_and_oracle_agree_on_the_shared_definitions():
    from artiboost_amd import draw as D
    f = ds.hand_faces()
    for a, b in zip(D.face_adjacency(f), do.adjacency(f)):
        assert np.array_equal(a, b)
    Rv, off, focal = D.orbit_rotation(224)
    Ro, pos, fo_ = do.orbit_camera(np.zeros(3), 224)
    assert np.array_equal(Rv, Ro) and np.array_equal(off, pos) and focal == fo_
    img = np.random.default_rng(1).uniform(-0.5, 0.5, (2, 3, 8, 8)).astype(np.float32)
    assert np.array_equal(D.frame_bytes(img)[1], do.frame_bytes(img[1]))


# ---- submit wiring
class _Fitter:
    def __call__(self, inp, pred_joints):
        B = pred_joints.shape[0]
        pj = pred_joints.detach().cpu().numpy()
        return [np.full((778, 3), float(pj[b, 0, 2])) for b in range(B)], [pj[b] + 1.0 for b in range(B)]


class _Drawer:
    def __init__(self):
        self.calls = []

    def draw_batch(self, image, cam_intr, sample_idx, pred_joints, fitted_verts, pred_obj_rotmat, pred_obj_tsl, pred_obj_corners, dataset,
                   draw_path, counter):
        os.makedirs(draw_path, exist_ok=True)
        self.calls.append(dict(n=image.shape[0], counter=counter, joints=pred_joints.clone(), verts=fitted_verts, rot=pred_obj_rotmat,
                               tsl=pred_obj_tsl, corners=pred_obj_corners, dataset=dataset, cam=cam_intr, idx=sample_idx))
        for _ in range(image.shape[0]):
            open(os.path.join(draw_path, f"{counter:0>4}.png"), "wb").close()
            counter += 1
        return counter


class _Model:
    def eval(self):
        return self

    def __call__(self, batch):
        B = batch["image"].shape[0]
        return {"m": {"joints_3d_abs": batch["j"].clone(), "box_rot_rotmat": torch.eye(3).repeat(B, 1, 1), "boxroot_3d_abs": batch["j"][:, :1] * 2,
                      "corners_3d_abs": batch["j"][:, :8] + 0.5}}


def _loader(sizes):
    g = torch.Generator().manual_seed(0)
    out, s = [], 0
    for n in sizes:
        out.append({"image": torch.rand((n, 3, 8, 8), generator=g) - 0.5, "cam_intr": torch.eye(3).repeat(n, 1, 1), "j": torch.randn((n, 21, 3), generator=g),
                    "root_joint": torch.randn((n, 3), generator=g), "sample_idx": torch.arange(s, s + n)})
        s += n
    return out


def _pass(cfg, tmp_path, name, sizes=(3, 5, 1)):
    from artiboost_amd.submit import HOSubmitEpochPass
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sp = HOSubmitEpochPass(cfg)
    dump = str(tmp_path / f"{name}.json")
    sp(0, _loader(sizes), _Model(), dump_path=dump, draw_path=str(tmp_path / name / "rendered_image"))
    return sp, json.load(open(dump)), str(tmp_path / name / "rendered_image")


def test_submit_pass_draws_every_frame_with_the_reference_arguments(tmp_path):
    dr = _Drawer()
    sp, js, path = _pass({"FIT_MESH": True, "DRAW": True, "TRUE_ROOT": True, "FITTING_UNIT": _Fitter(), "DRAWER": dr}, tmp_path, "draw")
    assert sorted(os.listdir(path)) == ["%04d.png" % i for i in range(9)]
    assert [c["n"] for c in dr.calls] == [3, 5, 1] and [c["counter"] for c in dr.calls] == [0, 3, 8] and sp.sample_counter == 9
    for c, b in zip(dr.calls, _loader((3, 5, 1))):
        assert torch.equal(c["joints"][:, 0], b["root_joint"]) and torch.equal(c["joints"][:, 1:], b["j"][:, 1:])      # true root substituted
        assert torch.equal(c["tsl"], b["j"][:, 0] * 2) and c["tsl"].shape == (c["n"], 3)
        assert torch.equal(c["corners"], b["j"][:, :8] + 0.5) and torch.equal(c["rot"], torch.eye(3).repeat(c["n"], 1, 1))
        assert torch.equal(c["idx"], b["sample_idx"]) and torch.equal(c["cam"], b["cam_intr"])
        assert len(c["verts"]) == c["n"] and c["verts"][0].shape == (778, 3)
    # the CodaLab file does not change with drawing
    _, plain, _ = _pass({"FIT_MESH": True, "TRUE_ROOT": True, "FITTING_UNIT": _Fitter()}, tmp_path, "plain")
    assert js == plain
    # DRAW without FIT_MESH: nothing is written, no drawer is asked
    dr2 = _Drawer()
    _, _, p2 = _pass({"DRAW": True, "DRAWER": dr2}, tmp_path, "nofit")
    assert not dr2.calls and not os.path.exists(p2)
    # DRAW_PATH overrides the directory
    dr3 = _Drawer()
    _pass({"FIT_MESH": True, "DRAW": True, "FITTING_UNIT": _Fitter(), "DRAWER": dr3, "DRAW_PATH": str(tmp_path / "elsewhere")}, tmp_path, "over")
    assert len(os.listdir(tmp_path / "elsewhere")) == 9


def test_constructor_warning_tells_the_truth():
    from artiboost_amd.submit import HOSubmitEpochPass
    with pytest.warns(UserWarning, match="postprocess_draw") as rec:
        sp = HOSubmitEpochPass({"FIT_MESH": True, "DRAW": True, "FITTING_UNIT": _Fitter()})
    assert len(rec) == 1 and "not pixel-comparable" in str(rec[0].message) and "not built" not in str(rec[0].message)
    assert ("skipped" in str(rec[0].message)) == (not torch.cuda.is_available()) == (not sp.draw)
    assert sp.drawer is None                                        # built at the first batch


# ---- MeshDrawer's host half, the kernel replaced by the oracle
def _oracle_drawer(monkeypatch, size=64):
    from artiboost_amd import draw as D
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    dr = D.MeshDrawer.__new__(D.MeshDrawer)
    dr.dev, dr.image_size, dr.hand_faces = torch.device("cpu"), (size, size), ds.hand_faces()
    dr._slot, dr._meshes, dr.tables = {}, [], {}

    def rasterise(image, cam_intr, fitted_verts, obj_id, obj_rot, obj_tsl, corners):
        image = image.numpy()
        B, _, H, W = image.shape
        sheet, cam = np.zeros((B, H, 4 * W, 3), np.uint8), np.zeros((B, 3), np.float32)
        for b in range(B):
            obj = dict(corners=corners[b].numpy()) if obj_id[b] == D.OBJ_BOX else None
            p2, p3, _, vs = do.draw_sample(np.asarray(fitted_verts[b]), dr.hand_faces, cam_intr[b].numpy(), image[b], obj)
            sheet[b, :, W:2 * W], sheet[b, :, 2 * W:3 * W], cam[b] = p2, p3, vs["orbit"][1]
        return sheet, cam
    dr.rasterise = rasterise
    return dr


def test_mesh_drawer_host_half_and_both_png_paths(monkeypatch, tmp_path):
    from PIL import Image
    from artiboost_amd import draw as D
    size = 64
    dr = _oracle_drawer(monkeypatch, size)
    sc = ds.make(2, 4, size)
    joints = torch.from_numpy(sc["hand_verts"][:, :21].copy())
    n = dr.draw_batch(torch.from_numpy(sc["image"]), torch.from_numpy(sc["cam_intr"]), torch.arange(2), joints, [v for v in sc["hand_verts"]], None, None,
                      torch.from_numpy(sc["corners"]), None, str(tmp_path), 7)
    assert n == 9 and sorted(os.listdir(tmp_path)) == ["0007.png", "0008.png"]
    img = np.asarray(Image.open(tmp_path / "0007.png").convert("RGB"))
    assert img.shape == (size, 4 * size, 3)
    frame = do.frame_bytes(sc["image"][0])
    p1, p2, p3, p4 = (img[:, k * size:(k + 1) * size] for k in range(4))
    assert (p1 != frame).any() and (p1 == frame).all(-1).mean() > 0.3              # a skeleton over the frame
    assert (p4 != 255).any() and (p4 == 255).all(-1).mean() > 0.3                  # a skeleton on white
    want2, want3, _, _ = do.draw_sample(sc["hand_verts"][0], dr.hand_faces, sc["cam_intr"][0], sc["image"][0], dict(corners=sc["corners"][0]))
    assert np.array_equal(p2, want2) and np.array_equal(p3, want3)
    # the module's own writer: decodes (Pillow, and this build's PNG reader) to the written bytes
    data = D.encode_png(img)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")), img)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import png_oracle as po
    assert np.array_equal(po.decode(data), img)
    D.write_png(str(tmp_path / "z.png"), img, use_pillow=False)
    D.write_png(str(tmp_path / "p.png"), img, use_pillow=True)
    assert open(tmp_path / "z.png", "rb").read() == data
    assert np.array_equal(np.asarray(Image.open(tmp_path / "z.png")), np.asarray(Image.open(tmp_path / "p.png")))
    assert np.array_equal(po.decode(open(tmp_path / "p.png", "rb").read()), img)


def test_ho3d_get_obj_faces_on_the_fake_tree(tmp_path, monkeypatch):
    import ho3d_fake_tree as ft
    from artiboost_amd import datasets as DS
    from test_ho3d_reader import PRESET
    tree = tmp_path / "tree"
    ft.build(str(tree), seed=7)
    monkeypatch.chdir(tmp_path)                                     # the annotation cache goes to ./common/cache
    d = DS.HO3D(DATA_ROOT=str(tree), DATA_SPLIT="test", SPLIT_MODE="paper", AUG=False, AUG_PARAM=None, DATA_PRESET=dict(PRESET, CROP_MODEL="hand_obj"))
    assert len(d) == 5
    rng = np.random.default_rng(7)
    written = {}
    for o in ft.OBJS:                                               # the tree's own draws: vertices, then 50 faces, per object
        ft._obj_verts(rng)
        written[o] = rng.integers(0, 200, (50, 3))
    for i, (seq, _) in enumerate([(s, k) for s, n, _ in ft.TEST for k in range(n)]):
        obj = dict((s, o) for s, _, o in ft.TEST)[seq]
        f = d.get_obj_faces(i)
        v, centre, _ = d.get_obj_verts_can(i)
        assert f.dtype == np.int32 and np.array_equal(f, written[obj])
        assert v.dtype == np.float32 and v.shape == (200, 3) and f.max() < len(v)
        np.testing.assert_allclose(v.min(0) + v.max(0), 0, atol=1e-6)          # centred on its bounding box
        assert d.get_obj_idx(i) == d.get_annots(i)["obj_idx"]
    assert d.get_obj_faces(0) is d.get_obj_faces(1)                 # read once per object


def test_exempt_sets_of_the_end_to_end_scenes_stay_under_the_cap():
    B, seed, size = ds.E2E
    sc, lib, hf = ds.make(B, seed, size), ds.library(), ds.hand_faces()
    for b in range(B):
        _, _, keys, vs = do.draw_sample(sc["hand_verts"][b], hf, sc["cam_intr"][b], sc["image"][b], ds.oracle_obj(sc, b, lib))
        for v in (0, 1):
            assert do.exempt_mask(vs, v, keys[v], size, size, ds.DEPTH_LEVELS).mean() <= ds.EXEMPT_CAP, (b, v)
