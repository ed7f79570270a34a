"""TEST INFRASTRUCTURE -- the seeded scenes of tests/test_gpu_draw.py and of the exemption-cap check in tests/test_draw_host.py: fitted hands
from tests/golden/mano_fit.npz placed 0.3 - 0.8 m in front of seeded cameras, objects with seeded poses (the stand-in library of
artiboost_amd/assets.py, a small octahedron for the mixed sizes), `obj_id = -1`, the box fallback, a hand partly outside the frame and one
entirely behind the camera."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ_NONE, OBJ_BOX = -1, -2


def hand_faces():
    from artiboost_amd.draw import hand_model_faces
    from artiboost_amd.hpregnet import load_hand_model
    return hand_model_faces(load_hand_model(None))


def library():
    """-> dict(ids, verts, faces, normals): the four stand-in HO3D objects (2048 vertices each) and an 8-face octahedron."""
    from artiboost_amd.assets import SceneAssets
    from artiboost_amd.draw import vertex_normals
    a = SceneAssets("HO3D", seed=1)
    verts = [np.asarray(o["verts"], np.float32) for o in a.objects]
    faces = [np.asarray(o["faces"], np.int32) for o in a.objects]
    verts.append(0.04 * np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32))
    faces.append(np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32))
    return dict(ids=list(range(len(verts))), verts=verts, faces=faces, normals=[vertex_normals(v, f).astype(np.float32) for v, f in zip(verts, faces)])


def make(B, seed, size=128):
    """-> dict of float32 / int32 arrays: hand_verts [B,778,3], cam_intr [B,3,3], image [B,3,H,W] (bytes / 255 - 0.5: the frame's bytes come
    back exactly), obj_id [B], obj_rot [B,3,3], obj_tsl [B,3], corners [B,8,3]."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "mano_fit.npz"))
    hands = g["mano_de_verts"]
    rng = np.random.default_rng(seed)
    W = H = size
    hv, Ks = np.zeros((B, 778, 3), np.float32), np.zeros((B, 3, 3), np.float32)
    obj_id, rot, tsl, corners = np.zeros(B, np.int32), np.zeros((B, 3, 3), np.float32), np.zeros((B, 3), np.float32), np.zeros((B, 8, 3), np.float32)
    n_lib = 5
    for b in range(B):
        v = hands[(b + seed) % len(hands)]
        v = v - v.mean(0)
        v = v * (0.09 / np.abs(v).max())                                 # a hand of about 18 cm, whatever the golden's unit
        f = rng.uniform(1.4, 2.2) * W
        c = np.array([rng.uniform(-0.03, 0.03), rng.uniform(-0.03, 0.03), rng.uniform(0.3, 0.8)])
        if B > 2 and b == 1:
            c[0] = 0.5 * W / f * c[2]                                    # centred on the right border: partly outside the frame
        if B > 2 and b == 2:
            c[2] = -0.4                                                  # entirely behind the camera
        hv[b] = v + c
        Ks[b] = [[f, 0, W / 2 + rng.uniform(-4, 4)], [0, f * rng.uniform(0.98, 1.02), H / 2 + rng.uniform(-4, 4)], [0, 0, 1]]
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        rot[b] = q * np.sign(np.linalg.det(q))
        tsl[b] = c + rng.uniform(-0.04, 0.04, 3)
        ext = rng.uniform(0.03, 0.07, 3)
        box = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * ext
        corners[b] = box @ rot[b].T + tsl[b]
        obj_id[b] = (list(range(n_lib)) + [OBJ_NONE, OBJ_BOX])[b % (n_lib + 2)]
    img = rng.integers(0, 256, (B, 3, H, W)).astype(np.float32) / np.float32(255.0) - np.float32(0.5)
    return dict(hand_verts=hv, cam_intr=Ks, image=img, obj_id=obj_id, obj_rot=rot, obj_tsl=tsl, corners=corners)


def oracle_obj(sc, b, lib):
    """The `obj` argument of draw_oracle.vertex_stage for sample b."""
    o = int(sc["obj_id"][b])
    if o == OBJ_NONE:
        return None
    if o == OBJ_BOX:
        return dict(corners=sc["corners"][b])
    return dict(verts_can=lib["verts"][o], normals_can=lib["normals"][o], faces=lib["faces"][o], R=sc["obj_rot"][b], t=sc["obj_tsl"][b])


# the end-to-end scenes: (B, seed, panel size); their exempt sets are held under the cap by tests/test_draw_host.py
E2E = (7, 11, 256)
# derived in tests/test_gpu_draw.py: the fp32 vertex stage's view-depth bound in 24-bit inverse-depth levels for z >= 0.2 m
DEPTH_LEVELS = 12
EXEMPT_CAP = 0.005
