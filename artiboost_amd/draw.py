"""Qualitative drawings of the submission pass (`--postprocess_fit_mesh --postprocess_draw`): anakin/viztools/draw.py:400-449
(save_a_image_with_mesh_joints_objects) as called by hodata_submit_epoch_pass.py:176-218 -- one PNG per test frame, four panels side
by side: skeleton overlay | mesh overlay | 3-D mesh | 3-D skeleton.

The reference draws the two mesh panels with OpenDR and mayavi (VTK, PyQt5, a connected X display), one sample at a time on the host.
Here `ab_draw_meshes` (csrc/draw.hip) rasterises both mesh panels of the WHOLE batch in one call from the device tensors the fit left
behind; the sheet comes to the host in one copy, the two skeleton panels are drawn there with PIL the way `metrics.Vis2DMetric._draw`
draws skeletons, and the files are written with Pillow (or, where it does not import, the zlib writer below: same pixels).

These drawings are this build's own: they are not pixel-comparable with the reference's.  The kernel needs a
HIP device; there is no CPU path."""
import os
import struct
import zlib

import numpy as np
import torch

from . import kernels as K
from .metrics import Vis2DMetric
from .registry import CONST

AZIMUTH, ELEVATION, DISTANCE, VIEW_ANGLE = -50.0, 50.0, 0.6, 30.0       # draw.py:264 / :223, mayavi's default view angle
DEXYCB_CORNER_ORDER = [0, 1, 3, 2, 4, 5, 7, 6]                         # hodata_submit_epoch_pass.py:186-187
OBJ_NONE, OBJ_BOX = -1, -2


def hand_model_faces(hand_model):
    """The 1538 faces of a hand model over its 778 vertices (the stand-in lists them over UV-seam duplicates: mapped back)."""
    f = np.asarray(hand_model["faces"])
    return np.asarray(hand_model["map"])[f].astype(np.int32) if "map" in hand_model else f.astype(np.int32)


def face_adjacency(faces, nverts=778):
    """CSR vertex -> faces table (ascending face index per vertex): the gather order of the kernel's vertex normals."""
    faces = np.asarray(faces).reshape(-1, 3)
    order = np.argsort(faces.reshape(-1), kind="stable")
    off = np.zeros(nverts + 1, np.int32)
    np.cumsum(np.bincount(faces.reshape(-1), minlength=nverts), out=off[1:])
    return off, (order // 3).astype(np.int32)


def vertex_normals(verts, faces):
    """Unit area-weighted vertex normals (float64), zero where no face meets."""
    verts = np.asarray(verts, np.float64)
    fn = np.cross(verts[faces[:, 1]] - verts[faces[:, 0]], verts[faces[:, 2]] - verts[faces[:, 0]])
    n = np.zeros_like(verts)
    for k in range(3):
        np.add.at(n, faces[:, k], fn)
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(ln > 0, n / np.where(ln > 0, ln, 1.0), 0.0)


def orbit_rotation(H):
    """Rows right / down / forward of the orbit camera, its offset from the look-at point and its focal length in pixels
    (mayavi's azimuth / elevation in the data frame, z up; 30 degree view angle over H pixels)."""
    az, el = np.radians(AZIMUTH), np.radians(ELEVATION)
    u = np.array([np.sin(el) * np.cos(az), np.sin(el) * np.sin(az), np.cos(el)])
    f = -u
    r = np.cross(f, [0.0, 0.0, 1.0])
    r /= np.linalg.norm(r)
    return np.stack([r, np.cross(f, r), f]), DISTANCE * u, 0.5 * H / np.tan(np.radians(VIEW_ANGLE / 2))


def encode_png(rgb):
    """Minimal PNG of a uint8 [H,W,3] array: 8-bit RGB, filter 0 on every line, one IDAT."""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    h, w = rgb.shape[:2]
    raw = np.concatenate([np.zeros((h, 1), np.uint8), rgb.reshape(h, w * 3)], 1).tobytes()

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 1)) +
            chunk(b"IEND", b""))


def write_png(path, rgb, use_pillow=None):
    """Pillow when it imports (use_pillow None), else the writer above; both decode to the same pixels."""
    if use_pillow is None:
        try:
            import PIL.Image  # noqa: F401
            use_pillow = True
        except ImportError:
            use_pillow = False
    if use_pillow:
        from PIL import Image
        Image.fromarray(np.ascontiguousarray(rgb, np.uint8)).save(path, format="PNG", compress_level=1)
    else:
        with open(path, "wb") as f:
            f.write(encode_png(rgb))


def frame_bytes(image):
    """float [B,3,H,W] (frame - 0.5) -> uint8 [B,H,W,3], floor(255 (image + 0.5) + 0.5) in float32: the kernel's uncovered pixels."""
    v = (np.asarray(image, np.float32) + np.float32(0.5)) * np.float32(255.0) + np.float32(0.5)
    return np.clip(np.floor(v), 0, 255).astype(np.uint8).transpose(0, 2, 3, 1)


def draw_skeleton(tile, joints_uv, corners_uv, joint_outline=(255, 255, 255)):
    """Hand skeleton and object box on a PIL image, as metrics.Vis2DMetric._draw: finger colours, CONST.JOINTS_IDX_PARENTS, box edges."""
    from PIL import ImageDraw
    d = ImageDraw.Draw(tile)
    ok = lambda *p: all(np.isfinite(q).all() and np.abs(q).max() < 1e5 for q in p)      # noqa: E731
    j = joints_uv
    for k in range(1, CONST.NUM_JOINTS):
        par = CONST.JOINTS_IDX_PARENTS[k]
        if ok(j[par], j[k]):
            d.line([tuple(j[par]), tuple(j[k])], fill=Vis2DMetric.FINGER_COLORS[(k - 1) // 4], width=2)
    for k in range(CONST.NUM_JOINTS):
        if ok(j[k]):
            d.ellipse([j[k][0] - 2, j[k][1] - 2, j[k][0] + 2, j[k][1] + 2], outline=joint_outline)
    if corners_uv is not None:
        c = corners_uv
        for a, b in Vis2DMetric.BOX_EDGES:
            if ok(c[a], c[b]):
                d.line([tuple(c[a]), tuple(c[b])], fill=(64, 224, 208), width=2)
    return tile


def _pinhole(P, intr):
    """hodata_submit_epoch_pass.py:199-203: (K P^T)^T, divided by its third column; points at z <= 0 become non-finite."""
    q = np.asarray(P, np.float64) @ np.asarray(intr, np.float64).T
    z = np.where(q[:, 2:3] > 1e-6, q[:, 2:3], np.nan)
    return q[:, :2] / z


class MeshDrawer:
    """`draw_batch` turns one batch of the submit pass into PNG contact sheets.  hand_faces [F,3]: the shared hand topology (MANO's
    1538 faces, or the closed-wrist faces of assets/postprocess/hand_close.npy).  object_library: None (built lazily from the dataset's
    get_obj_verts_can / get_obj_faces / get_obj_idx, cached per object) or a dict(verts=[...], faces=[...], ids=[...]) of canonical meshes.
    `rasterise(...)` is the device half (ab_draw_meshes); tests replace it."""

    def __init__(self, hand_faces, object_library=None, image_size=(256, 256), device="cuda"):
        if not torch.cuda.is_available():
            raise RuntimeError("--postprocess_draw rasterises on a HIP device (ab_draw_meshes) and none is visible; there is no CPU path")
        self.dev = torch.device(device)
        self.image_size = tuple(image_size)
        self.hand_faces = np.ascontiguousarray(np.asarray(hand_faces).reshape(-1, 3), np.int32)
        if self.hand_faces.min() < 0 or self.hand_faces.max() >= 778:
            raise ValueError("hand_faces index outside the 778 MANO vertices")
        off, adj = face_adjacency(self.hand_faces)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)      # noqa: E731
        self._hand = dict(hand_faces=t(self.hand_faces), adj_off=t(off), adj_face=t(adj))
        self.tables = dict(self._hand, n_obj=0)
        self._slot, self._meshes = {}, []
        if object_library:
            for oid, v, f in zip(object_library["ids"], object_library["verts"], object_library["faces"]):
                self._add_object(oid, v, f)
            self._upload()

    # ---- object library
    def _add_object(self, oid, verts, faces):
        verts, faces = np.asarray(verts, np.float32).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3)
        if len(faces) and (faces.min() < 0 or faces.max() >= len(verts)):
            raise ValueError(f"object {oid}: face index outside its {len(verts)} vertices")
        self._slot[oid] = len(self._meshes)
        self._meshes.append((verts, faces, vertex_normals(verts, faces).astype(np.float32)))

    def _upload(self):
        vo = np.cumsum([0] + [len(m[0]) for m in self._meshes]).astype(np.int32)
        fo = np.cumsum([0] + [len(m[1]) for m in self._meshes]).astype(np.int32)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)      # noqa: E731
        self.tables = dict(self._hand, n_obj=len(self._meshes), obj_verts=t(np.concatenate([m[0] for m in self._meshes])),
                           obj_normals=t(np.concatenate([m[2] for m in self._meshes])), obj_faces=t(np.concatenate([m[1] for m in self._meshes])),
                           obj_vert_off=t(vo), obj_face_off=t(fo), max_obj_verts=int(np.diff(vo).max()), max_obj_faces=int(np.diff(fo).max()))

    def object_ids(self, dataset, sample_idx, have_corners):
        """Per sample: the library slot of its object (meshes read from the dataset once per object), OBJ_BOX when the dataset has no
        meshes but corners were predicted, OBJ_NONE otherwise."""
        if dataset is None or not all(hasattr(dataset, a) for a in ("get_obj_faces", "get_obj_verts_can", "get_obj_idx")):
            return np.full(len(sample_idx), OBJ_BOX if have_corners else OBJ_NONE, np.int32)
        out, grew = np.zeros(len(sample_idx), np.int32), False
        for n, i in enumerate(sample_idx):
            oid = int(dataset.get_obj_idx(int(i)))
            if oid not in self._slot:
                self._add_object(oid, dataset.get_obj_verts_can(int(i))[0], dataset.get_obj_faces(int(i)))
                grew = True
            out[n] = self._slot[oid]
        if grew:
            self._upload()
        return out

    # ---- device half
    def rasterise(self, image, cam_intr, fitted_verts, obj_id, obj_rot, obj_tsl, corners):
        """-> (sheet uint8 [B,H,4W,3] with panels 2 and 3 filled and panels 1, 4 zero, orbit camera positions float [B,3]), on the host:
        ONE device-to-host copy (the positions ride behind the sheet in the same buffer)."""
        dev, B, H, W = self.dev, image.shape[0], image.shape[2], image.shape[3]
        f32 = lambda a: torch.as_tensor(a).to(dev, torch.float32).contiguous()      # noqa: E731
        n = B * H * 4 * W * 3
        buf = torch.zeros((n + B * 16,), dtype=torch.uint8, device=dev)
        cam = K.draw_meshes(f32(fitted_verts), self.tables, f32(image), f32(cam_intr), buf[:n].view(B, H, 4 * W, 3),
                            obj_id=torch.as_tensor(obj_id).to(dev, torch.int32).contiguous(), obj_rot=f32(obj_rot), obj_tsl=f32(obj_tsl),
                            corners=f32(corners) if corners is not None else None)
        buf[n:] = cam.reshape(-1).view(torch.uint8)
        host = buf.cpu().numpy()
        return host[:n].reshape(B, H, 4 * W, 3), host[n:].view(np.float32).reshape(B, 4)[:, :3]

    # ---- the whole batch
    def draw_batch(self, image, cam_intr, sample_idx, pred_joints, fitted_verts, pred_obj_rotmat, pred_obj_tsl, pred_obj_corners, dataset,
                   draw_path, counter):
        """hodata_submit_epoch_pass.py:176-218 for one batch; -> the counter after it.  image float [B,3,H,W] (frame - 0.5); fitted_verts a
        device tensor [B,778,3] (FittingUnit.fit) or a list of arrays.  Files `{counter:0>4}.png` under draw_path."""
        from PIL import Image
        os.makedirs(draw_path, exist_ok=True)
        host = lambda a: None if a is None else torch.as_tensor(a).detach().float().cpu().numpy()      # noqa: E731
        if not torch.is_tensor(fitted_verts):
            fitted_verts = torch.from_numpy(np.stack([np.asarray(v, np.float32) for v in fitted_verts]))
        image = torch.as_tensor(image).detach()
        B, H, W = image.shape[0], image.shape[2], image.shape[3]
        joints, corners, intr = host(pred_joints), host(pred_obj_corners), host(cam_intr)
        if corners is not None and getattr(dataset, "name", None) == "DexYCB":
            corners = corners[:, DEXYCB_CORNER_ORDER]
        idx = [int(i) for i in torch.as_tensor(sample_idx).reshape(-1).tolist()] if sample_idx is not None else list(range(B))
        obj_id = self.object_ids(dataset, idx, corners is not None)
        rot = pred_obj_rotmat if pred_obj_rotmat is not None else torch.eye(3).repeat(B, 1, 1)
        tsl = pred_obj_tsl if pred_obj_tsl is not None else torch.zeros(B, 3)
        sheet, cam_pos = self.rasterise(image, torch.as_tensor(cam_intr), fitted_verts, obj_id, torch.as_tensor(rot).detach(),
                                        torch.as_tensor(tsl).detach(), None if corners is None else torch.from_numpy(np.ascontiguousarray(corners)))
        sheet = np.array(sheet, np.uint8)
        frames = frame_bytes(image.float().cpu().numpy())
        Rv, _, focal = orbit_rotation(H)
        for b in range(B):
            # panel 1: the skeleton over the frame, from cam_intr-projected joints / corners
            p1 = draw_skeleton(Image.fromarray(frames[b]), _pinhole(joints[b], intr[b]), None if corners is None else _pinhole(corners[b], intr[b]))
            sheet[b, :, :W] = np.asarray(p1)
            # panel 4: the same skeleton on white through panel 3's orbit camera
            Kv = np.array([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1.0]])
            view = lambda P: _pinhole((np.asarray(P, np.float64) - cam_pos[b].astype(np.float64)) @ Rv.T, Kv)      # noqa: E731
            p4 = draw_skeleton(Image.new("RGB", (W, H), (255, 255, 255)), view(joints[b]), None if corners is None else view(corners[b]),
                               joint_outline=(64, 64, 64))
            sheet[b, :, 3 * W:] = np.asarray(p4)
            write_png(os.path.join(draw_path, f"{counter:0>4}.png"), sheet[b])
            counter += 1
        return counter
