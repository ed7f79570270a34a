"""ab_draw_meshes (csrc/draw.hip) and the drawing path of the submit pass on the device, against tests/draw_oracle.py.  Scenes:
tests/draw_scenes.py.  The output sheet is prefilled with a sentinel byte.

  vertex stage   the kernel's vertex records against the float64 oracle: snapped screen coordinates within +-1 unit of 1/256 px, view depth
                 and lit colour within bounds derived below from the fp32 operation count
  raster stage   teacher-forced: the integer oracle, fed the DEVICE's snapped coordinates and depths, names the same winning face (and
                 depth) at every pixel of both panels, B = 1, 37, 64, 100
  end to end     from float inputs: every pixel outside the oracle-defined exempt set within +-1 level; uncovered pixels exact; panels
                 1 and 4 untouched
  determinism    two runs, and runs beside an MFMA-heavy kernel on another stream, give the same bytes
  contracts      the dispatcher refuses short buffers and wrong dtypes
  submit         train/submit_reload.py --postprocess_fit_mesh --postprocess_draw writes one PNG per frame and the same json

Bounds (U = 2^-24, the fp32 unit roundoff; every coordinate of a scene is below 2 m in magnitude):
  view depth     object transform (5 roundings), camera offset (1), rotation row (5): <= 11 roundings of values <= 2 m, taken as
                 16 U * 2 m = 1.9e-6 m.
  depth level    one level of the 24-bit inverse depth is 99.99 / 2^24 = 5.96e-6 1/m.  The depth error moves 1/z by 1.9e-6 / z^2: at
                 z >= 0.2 m that is under 8 levels.  The quantisation itself, in fp32: 1/z - 100 is rounded at magnitude 100 (half an
                 ulp = 3.8e-6: 0.64 level), the division by -99.99 and the product with 2^24 - 1 each round a value of up to 2^24
                 levels to half an ulp (1 and 0.5 level), then + 0.5 and floor (1 level): under 4 levels.  Bound: 1.9e-6 / z^2 in
                 levels + 4; for z >= 0.2 m, 12 levels (draw_scenes.DEPTH_LEVELS, the depth half of the exempt set).
  lit colour     normal: <= 16 gathered cross products (9 roundings each, then the running sum), normalisation (7), per light a
                 direction (9), a dot product (5), two divisions, the sum of three lights (3), the base colour and the clamp (2):
                 under 256 roundings in all, of values <= 2.7 (the three light colours): 256 U * 2.7 = 4.2e-5, far below one
                 8-bit level (3.9e-3)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import draw_oracle as do
import draw_scenes as ds

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
DEPTH_BOUND = 16 * U * 2.0
COLOR_BOUND = 256 * U * 2.7
SENTINEL = 0x5A


def _drawer(size):
    from artiboost_amd.draw import MeshDrawer
    lib = ds.library()
    return MeshDrawer(ds.hand_faces(), object_library=lib, image_size=(size, size)), lib


def _run(drawer, sc, debug=True):
    from artiboost_amd import kernels as K
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    B, _, H, W = sc["image"].shape
    out = torch.full((B, H, 4 * W, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    r = K.draw_meshes(t(sc["hand_verts"]), drawer.tables, t(sc["image"]), t(sc["cam_intr"]), out, obj_id=t(sc["obj_id"]), obj_rot=t(sc["obj_rot"]),
                      obj_tsl=t(sc["obj_tsl"]), corners=t(sc["corners"]), debug=debug)
    torch.cuda.synchronize()
    if not debug:
        return out.cpu().numpy()
    cam, rec, keys = r
    return out.cpu().numpy(), cam.cpu().numpy(), rec.cpu().numpy(), keys.cpu().numpy().view(np.uint64)


def _views(rec):
    """Vertex records int32 [V,12] -> per view dict(sx, sy, zq, zv, ok), colour [V,3]."""
    f = rec.view(np.float32)
    fl = rec[:, 11]
    v = [dict(sx=rec[:, 0].astype(np.int64), sy=rec[:, 1].astype(np.int64), zq=rec[:, 2].astype(np.int64), zv=f[:, 6], ok=(fl & 1) != 0),
         dict(sx=rec[:, 3].astype(np.int64), sy=rec[:, 4].astype(np.int64), zq=rec[:, 5].astype(np.int64), zv=f[:, 7], ok=(fl & 2) != 0)]
    return v, f[:, 8:11]


def test_vertex_stage_against_float64():
    drawer, lib = _drawer(128)
    sc = ds.make(14, 3, 128)
    _, cam, rec, _ = _run(drawer, sc)
    hf = ds.hand_faces()
    worst = dict(xy=0, z=0.0, c=0.0)
    for b in range(14):
        vs = do.vertex_stage(sc["hand_verts"][b], hf, sc["cam_intr"][b], 128, 128, ds.oracle_obj(sc, b, lib))
        n = len(vs["P"])
        dv, col = _views(rec[b, :n])
        assert np.abs(cam[b, :3] - vs["orbit"][1]).max() <= 4 * U * 2.0
        for v in (0, 1):
            o, d = vs[v], dv[v]
            # usable flags agree except where the float64 depth is within the bound of the near plane
            sure = np.abs(o["zv"] - do.NEAR) > DEPTH_BOUND
            assert (o["ok"] == d["ok"])[sure].all()
            both = o["ok"] & d["ok"]
            worst["xy"] = max(worst["xy"], int(np.abs(o["sx"] - d["sx"])[both].max(initial=0)), int(np.abs(o["sy"] - d["sy"])[both].max(initial=0)))
            worst["z"] = max(worst["z"], float(np.abs(o["zv"] - d["zv"].astype(np.float64)).max()))
            lv = np.abs(o["zq"] - d["zq"])[both]
            assert (lv <= DEPTH_BOUND / o["zv"][both] ** 2 / ((do.NEAR_INV - do.FAR_INV) / do.ZMAX) + 4).all(), int(lv.max(initial=0))
        worst["c"] = max(worst["c"], float(np.abs(vs["color"] - col.astype(np.float64)).max()))
    print("vertex stage: worst |d snapped| %d units, |d depth| %.3g m (bound %.3g), |d colour| %.3g (bound %.3g)" %
          (worst["xy"], worst["z"], DEPTH_BOUND, worst["c"], COLOR_BOUND))
    assert worst["xy"] <= 1
    assert worst["z"] <= DEPTH_BOUND
    assert worst["c"] <= COLOR_BOUND


@pytest.mark.parametrize("B", [1, 37, 64, 100])
def test_raster_stage_teacher_forced(B):
    size = 256 if B == 1 else 96
    drawer, lib = _drawer(size)
    sc = ds.make(B, 100 + B, size)
    out, _, rec, keys = _run(drawer, sc)
    hf = ds.hand_faces()
    covered = 0
    for b in range(B):
        o = int(sc["obj_id"][b])
        faces = [hf.astype(np.int64)]
        if o == ds.OBJ_BOX:
            faces.append(do.BOX_FACES.astype(np.int64) + 778)
        elif o >= 0:
            faces.append(lib["faces"][o].astype(np.int64) + 778)
        faces = np.concatenate(faces)
        dv, _ = _views(rec[b])
        for v in (0, 1):
            d = dv[v]
            want = do.raster_stage(d["sx"], d["sy"], d["zq"], d["ok"], faces, size, size, len(hf) if v == 0 else None)
            bad = want != keys[b, v]
            assert not bad.any(), (B, b, v, int(bad.sum()), want[bad][:4], keys[b, v][bad][:4])
            covered += int((want != do.EMPTY).sum())
    assert covered > 0
    assert (out[:, :, :size] == SENTINEL).all() and (out[:, :, 3 * size:] == SENTINEL).all()
    if B > 2:
        assert (keys[2, 0] == do.EMPTY).all()                      # the hand behind the camera leaves the overlay to the frame
        np.testing.assert_array_equal(out[2, :, size:2 * size], do.frame_bytes(sc["image"][2]))


def test_end_to_end_pixels():
    B, seed, size = ds.E2E
    drawer, lib = _drawer(size)
    sc = ds.make(B, seed, size)
    out = _run(drawer, sc, debug=False)
    hf = ds.hand_faces()
    worst, nex = 0, 0.0
    for b in range(B):
        p2, p3, keys, vs = do.draw_sample(sc["hand_verts"][b], hf, sc["cam_intr"][b], sc["image"][b], ds.oracle_obj(sc, b, lib))
        for v, want in ((0, p2), (1, p3)):
            got = out[b, :, (1 + v) * size:(2 + v) * size]
            ex = do.exempt_mask(vs, v, keys[v], size, size, ds.DEPTH_LEVELS)
            assert ex.mean() <= ds.EXEMPT_CAP, (b, v, ex.mean())
            nex = max(nex, float(ex.mean()))
            diff = np.abs(got.astype(np.int32) - want.astype(np.int32)).max(-1)
            worst = max(worst, int(diff[~ex].max()))
            unc = (keys[v] == do.EMPTY) & ~ex
            bg = do.frame_bytes(sc["image"][b]) if v == 0 else np.full((size, size, 3), 255, np.uint8)
            assert (got[unc] == bg[unc]).all(), (b, v)
    print("end to end: worst difference outside the exempt set %d level(s); largest exempt set %.4f of a panel" % (worst, nex))
    assert worst <= 1
    assert (out[:, :, :size] == SENTINEL).all() and (out[:, :, 3 * size:] == SENTINEL).all()


def test_two_runs_are_bit_identical_also_beside_mfma_kernels():
    from artiboost_amd import kernels as K
    drawer, _ = _drawer(128)
    sc = ds.make(24, 5, 128)
    ref = _run(drawer, sc)
    again = _run(drawer, sc)
    for a, b in zip(ref, again):
        assert np.array_equal(a, b)
    x3, w3 = K.split(torch.randn(64, 16, 16, 256, device="cuda")), K.split(torch.randn(256, 3, 3, 256, device="cuda") * 0.05)
    K.conv2d_fwd_x3(x3, w3, 1, 1, want_stats=True)
    side = torch.cuda.Stream()
    for it in range(6):
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(10):
                K.conv2d_fwd_x3(x3, w3, 1, 1, want_stats=True)
        got = _run(drawer, sc)
        for name, a, b in zip(("sheet", "camera", "records", "keys"), ref, got):
            assert np.array_equal(a, b), (it, name)


def test_dispatcher_refuses_short_buffers_and_wrong_dtypes():
    from artiboost_amd import kernels as K
    drawer, _ = _drawer(64)
    sc = ds.make(3, 9, 64)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    out = torch.zeros((3, 64, 256, 3), dtype=torch.uint8, device="cuda")
    good = dict(obj_id=t(sc["obj_id"]), obj_rot=t(sc["obj_rot"]), obj_tsl=t(sc["obj_tsl"]), corners=t(sc["corners"]))
    K.draw_meshes(t(sc["hand_verts"]), drawer.tables, t(sc["image"]), t(sc["cam_intr"]), out, **good)
    with pytest.raises(RuntimeError, match="hand_verts"):
        K.draw_meshes(t(sc["hand_verts"][:2]), drawer.tables, t(sc["image"]), t(sc["cam_intr"]), out, **good)
    with pytest.raises(RuntimeError, match="cam_intr"):
        K.draw_meshes(t(sc["hand_verts"]), drawer.tables, t(sc["image"]), t(sc["cam_intr"][:1]), out, **good)
    with pytest.raises(RuntimeError, match="obj_id"):
        K.draw_meshes(t(sc["hand_verts"]), drawer.tables, t(sc["image"]), t(sc["cam_intr"]), out, **dict(good, obj_id=t(sc["obj_id"]).long()))
    with pytest.raises(RuntimeError, match="image"):
        K.draw_meshes(t(sc["hand_verts"]), drawer.tables, t(sc["image"]).double(), t(sc["cam_intr"]), out, **good)
    with pytest.raises(RuntimeError, match="corners"):
        K.draw_meshes(t(sc["hand_verts"]), drawer.tables, t(sc["image"]), t(sc["cam_intr"]), out, **dict(good, corners=t(sc["corners"][:2])))
    torch.cuda.synchronize()


def _submit(tmp, extra):
    cmd = [sys.executable, os.path.join(ROOT, "train", "submit_reload.py"), "--cfg", os.path.join(ROOT, "config", "eval_ho3dv2_clasbased_artiboost_mi355x.yaml"),
           "--batch_size", "4", "--submit_dump", "--random_frames", "6", "--ignore_pretrained", "--postprocess_fit_mesh"] + extra
    r = subprocess.run(cmd, cwd=str(tmp), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    jsons = [os.path.join(dp, f) for dp, _, fs in os.walk(str(tmp)) for f in fs if f.endswith("_SUBMIT.json")]
    assert len(jsons) == 1, jsons
    return jsons[0]


def test_submit_reload_draws_one_png_per_frame(tmp_path):
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, "train"))
    a, b = tmp_path / "plain", tmp_path / "draw"
    a.mkdir(), b.mkdir()
    ja, jb = _submit(a, []), _submit(b, ["--postprocess_draw"])
    assert json.load(open(ja)) == json.load(open(jb))
    pngs = sorted(os.path.join(dp, f) for dp, _, fs in os.walk(str(b)) for f in fs if f.endswith(".png") and os.path.basename(dp) == "rendered_image")
    assert [os.path.basename(p) for p in pngs] == ["%04d.png" % i for i in range(6)]
    assert not [f for dp, _, fs in os.walk(str(a)) for f in fs if f.endswith(".png") and os.path.basename(dp) == "rendered_image"]
    verts = np.asarray(json.load(open(jb))[1])
    import submit_reload as sr
    import yaml
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "eval_ho3dv2_clasbased_artiboost_mi355x.yaml")))
    size = cfg["DATA_PRESET"]["IMAGE_SIZE"]
    seed = cfg.get("TRAIN", {}).get("MANUAL_SEED", 1)
    batches = sr._random_batches(6, 4, size, seed)
    frames = np.concatenate([do.frame_bytes(im) [None] for bt in batches for im in bt["image"].numpy()])
    Ks = np.concatenate([bt["cam_intr"].numpy() for bt in batches])
    W, H = size
    for i, p in enumerate(pngs):
        img = np.asarray(Image.open(p).convert("RGB"))
        assert img.shape == (H, 4 * W, 3)
        p2 = img[:, W:2 * W]
        uv = (verts[i] @ Ks[i].T.astype(np.float64))
        uv = uv[:, :2] / uv[:, 2:3]
        x0, y0, x1, y1 = np.floor(uv[:, 0].min()) - 1, np.floor(uv[:, 1].min()) - 1, np.ceil(uv[:, 0].max()) + 1, np.ceil(uv[:, 1].max()) + 1
        yy, xx = np.mgrid[0:H, 0:W]
        inside = (xx >= x0) & (xx <= x1) & (yy >= y0) & (yy <= y1)
        same = (p2 == frames[i]).all(-1)
        assert same[~inside].all(), i
        if inside.any() and (verts[i][:, 2] > 0.01).all():
            assert not same[inside].all(), i
