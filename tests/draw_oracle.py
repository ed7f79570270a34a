"""TEST INFRASTRUCTURE -- the definition of the `--postprocess_draw` pixels in numpy: a float64 vertex stage
(object transform, both cameras, gathered area-weighted normals, three-light Lambert), an INTEGER raster stage over snapped screen
coordinates (coverage, depth winner, tie rule: exact) and float64 interpolation / quantisation.  csrc/draw.hip is held to this file by
tests/test_gpu_draw.py; tests/test_draw_host.py holds this file to closed forms.  Nothing here imports torch or the package."""
import numpy as np

HAND_VERTS = 778
HAND_COLOR = np.array([102.0, 209.0, 243.0]) / 255.0
OBJ_COLOR = np.array([255.0, 163.0, 172.0]) / 255.0
NEAR, NEAR_INV, FAR_INV, ZMAX = 0.01, 100.0, 0.01, 16777215.0
XY_LIMIT = 32768.0
AREA_LIMIT = 1 << 39
OBJ_NONE, OBJ_BOX = -1, -2
AZIMUTH, ELEVATION, DISTANCE, VIEW_ANGLE = -50.0, 50.0, 0.6, 30.0
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
# the box over 8 corners indexed 4 ix + 2 iy + iz, outward winding for a right-handed box
BOX_FACES = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1],
                      [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)


def lights():
    """opendr_renderer.py:137-170: the three positions as row vectors times R_y(120 degrees), light colours 1, 1, 0.7."""
    a = np.radians(120.0)
    ry = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    pos = np.array([[-200.0, -100.0, -100.0], [800.0, 10.0, 300.0], [-500.0, 500.0, 1000.0]]) @ ry
    return pos, np.array([1.0, 1.0, 0.7])


def orbit_camera(center, H):
    """mayavi's view(azimuth, elevation, distance) with the data frame taken as it is (z up): the camera sits at
    centre + distance * u, u = (sin el cos az, sin el sin az, cos el), looks along f = -u; right = normalize(f x z), down = f x right.
    -> (rotation rows right / down / forward, position, focal length in pixels for a VIEW_ANGLE vertical field of view of H pixels)."""
    az, el = np.radians(AZIMUTH), np.radians(ELEVATION)
    u = np.array([np.sin(el) * np.cos(az), np.sin(el) * np.sin(az), np.cos(el)])
    f = -u
    r = np.cross(f, [0.0, 0.0, 1.0])
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    return np.stack([r, d, f]), np.asarray(center, np.float64) + DISTANCE * u, 0.5 * H / np.tan(np.radians(VIEW_ANGLE / 2))


def adjacency(faces, nverts=HAND_VERTS):
    """CSR vertex -> faces table, ascending face index per vertex (the kernel's gather order)."""
    faces = np.asarray(faces)
    order = np.argsort(faces.reshape(-1), kind="stable")
    off = np.zeros(nverts + 1, np.int32)
    np.cumsum(np.bincount(faces.reshape(-1), minlength=nverts), out=off[1:])
    return off, (order // 3).astype(np.int32)


def vertex_normals(verts, faces):
    """Area-weighted sums of the face normals (cross products, not normalised)."""
    verts = np.asarray(verts, np.float64)
    fn = np.cross(verts[faces[:, 1]] - verts[faces[:, 0]], verts[faces[:, 2]] - verts[faces[:, 0]])
    n = np.zeros_like(verts)
    for k in range(3):
        np.add.at(n, faces[:, k], fn)
    return n


def lambert(P, n, base):
    """Per-vertex colour: base * sum_l colour_l * max(n^ . l^, 0), clamped to [0, 1]; a zero normal gives black."""
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    nh = np.where(ln > 0, n / np.where(ln > 0, ln, 1.0), 0.0)
    pos, col = lights()
    s = np.zeros(len(P))
    for p, c in zip(pos, col):
        d = p[None] - P
        s += c * np.maximum((nh * d).sum(1) / np.linalg.norm(d, axis=1), 0.0)
    return np.clip(base[None] * s[:, None], 0.0, 1.0)


def quant_z(Z):
    z01 = (1.0 / Z - NEAR_INV) / (FAR_INV - NEAR_INV)
    return np.clip(np.floor(z01 * ZMAX + 0.5), 0, ZMAX).astype(np.int64)


def project(fx, fy, cx, cy, Q):
    """-> (x, y float64 pixels, usable mask).  Unusable: z <= NEAR, or a coordinate at or beyond XY_LIMIT pixels."""
    Z = Q[:, 2]
    ok = Z > NEAR
    Zs = np.where(ok, Z, 1.0)
    x, y = fx * Q[:, 0] / Zs + cx, fy * Q[:, 1] / Zs + cy
    ok &= (np.abs(x) < XY_LIMIT) & (np.abs(y) < XY_LIMIT)
    return x, y, ok


def snap(x):
    return np.floor(x * 256.0 + 0.5).astype(np.int64)


def vertex_stage(hand_verts, hand_faces, K, W, H, obj=None):
    """One sample.  obj: None | dict(verts_can, normals_can, faces, R, t) | dict(corners).  -> dict: P [V,3], color [V,3], faces [F,3]
    (global vertex indices, hand first), nhf, and per view v in (0, 1): x / y float pixels, sx / sy snapped, zq, zv, ok."""
    hv = np.asarray(hand_verts, np.float64)
    hf = np.asarray(hand_faces, np.int64)
    P, col, faces = [hv], [lambert(hv, vertex_normals(hv, hf), HAND_COLOR)], [hf]
    if obj is not None:
        if "corners" in obj:
            ov = np.asarray(obj["corners"], np.float64)
            on, of = vertex_normals(ov, BOX_FACES), BOX_FACES
        else:
            R, t = np.asarray(obj["R"], np.float64), np.asarray(obj["t"], np.float64)
            ov = np.asarray(obj["verts_can"], np.float64) @ R.T + t
            on, of = np.asarray(obj["normals_can"], np.float64) @ R.T, np.asarray(obj["faces"])
        P.append(ov)
        col.append(lambert(ov, on, OBJ_COLOR))
        faces.append(np.asarray(of, np.int64) + HAND_VERTS)
    P = np.concatenate(P)
    out = dict(P=P, color=np.concatenate(col), faces=np.concatenate(faces), nhf=len(hf))
    K = np.asarray(K, np.float64)
    Rv, pos, focal = orbit_camera((P.min(0) + P.max(0)) / 2, H)
    out["orbit"] = (Rv, pos, focal)
    for v, (Q, intr) in enumerate(((P, (K[0, 0], K[1, 1], K[0, 2], K[1, 2])), ((P - pos) @ Rv.T, (focal, focal, W / 2, H / 2)))):
        x, y, ok = project(*intr, Q)
        out[v] = dict(x=x, y=y, ok=ok, sx=np.where(ok, snap(np.where(ok, x, 0)), 0), sy=np.where(ok, snap(np.where(ok, y, 0)), 0),
                      zq=np.where(ok, quant_z(np.where(ok, Q[:, 2], 1.0)), 0), zv=Q[:, 2])
    return out


def _oriented(sx, sy, zq, ok, faces):
    """Faces usable in this view, oriented to positive doubled area.  -> (face ids, vertex ids [n,3]), dropped: an unusable vertex,
    zero area, |area| >= AREA_LIMIT."""
    f = np.asarray(faces, np.int64)
    x, y = sx[f], sy[f]
    area = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])
    keep = ok[f].all(1) & (area != 0) & (np.abs(area) < AREA_LIMIT)
    ids = np.nonzero(keep)[0]
    f = f[ids].copy()
    neg = area[ids] < 0
    f[neg] = f[neg][:, [0, 2, 1]]
    return ids, f


def _edges(x, y, px, py):
    """Edge functions w0 (v1 v2), w1 (v2 v0), w2 (v0 v1) at (px, py), their shared-edge-rule biases; x, y [..., 3] broadcast against px, py."""
    w, bias = [], []
    for a, b in ((1, 2), (2, 0), (0, 1)):
        ex, ey = x[..., b] - x[..., a], y[..., b] - y[..., a]
        w.append(ex * (py - y[..., a]) - ey * (px - x[..., a]))
        bias.append(np.where((ey > 0) | ((ey == 0) & (ex < 0)), 0, 1))
    return w, bias


def raster_stage(sx, sy, zq, ok, faces, W, H, nfaces_drawn=None):
    """INTEGER raster of one view: keys uint64 [H, W] = depth << 32 | face id (EMPTY: uncovered).  sx, sy: snapped screen coordinates
    (1/256 px), zq: 24-bit depths, ok: usable vertices; faces [F,3]; only the first nfaces_drawn faces are drawn (the overlay: hand only).
    Pixel centres at (x + 0.5, y + 0.5); a centre on an edge belongs to the triangle by the shared-edge rule of oracle/render_oracle.c
    (edge (dx, dy) of the positively oriented triangle: dy > 0, or dy == 0 and dx < 0); depth = floor(sum w_k z_k / sum w_k); nearest wins, equal depth goes to the lower face index (the minimum of the keys)."""
    sx, sy, zq = (np.asarray(a, np.int64) for a in (sx, sy, zq))
    faces = np.asarray(faces)[:nfaces_drawn]
    keys = np.full(H * W, EMPTY, np.uint64)
    ids, f = _oriented(sx, sy, zq, np.asarray(ok, bool), faces)
    if not len(ids):
        return keys.reshape(H, W)
    x, y, z = sx[f], sy[f], zq[f]
    x0 = np.maximum(0, (x.min(1) - 128 + 255) >> 8)
    x1 = np.minimum(W - 1, (x.max(1) - 128) >> 8)
    y0 = np.maximum(0, (y.min(1) - 128 + 255) >> 8)
    y1 = np.minimum(H - 1, (y.max(1) - 128) >> 8)
    live = (x0 <= x1) & (y0 <= y1)
    span = np.maximum(x1 - x0, y1 - y0) + 1
    done = ~live
    for size in (2, 4, 8, 16, 32, 64):                       # faces whose pixel box fits size x size, all at once
        sel = np.nonzero(~done & (span <= size))[0]
        done[sel] = True
        if not len(sel):
            continue
        oy, ox = np.mgrid[0:size, 0:size]
        X = x0[sel, None] + ox.reshape(1, -1)
        Y = y0[sel, None] + oy.reshape(1, -1)
        inside = (X <= x1[sel, None]) & (Y <= y1[sel, None])
        w, bias = _edges(x[sel, None, :], y[sel, None, :], X * 256 + 128, Y * 256 + 128)
        cov = inside & (w[0] >= bias[0]) & (w[1] >= bias[1]) & (w[2] >= bias[2])
        num = w[0] * z[sel, None, 0] + w[1] * z[sel, None, 1] + w[2] * z[sel, None, 2]
        q = num // np.where(cov, w[0] + w[1] + w[2], 1)
        k = (q.astype(np.uint64) << np.uint64(32)) | np.broadcast_to(ids[sel, None], q.shape).astype(np.uint64)
        np.minimum.at(keys, (Y * W + X)[cov], k[cov])
    for i in np.nonzero(~done)[0]:                           # the few large ones, one at a time
        Y, X = np.mgrid[y0[i]:y1[i] + 1, x0[i]:x1[i] + 1]
        w, bias = _edges(x[i], y[i], X * 256 + 128, Y * 256 + 128)
        cov = (w[0] >= bias[0]) & (w[1] >= bias[1]) & (w[2] >= bias[2])
        num = w[0] * z[i, 0] + w[1] * z[i, 1] + w[2] * z[i, 2]
        q = num[cov] // (w[0] + w[1] + w[2])[cov]
        np.minimum.at(keys, (Y * W + X)[cov], (q.astype(np.uint64) << np.uint64(32)) | np.uint64(ids[i]))
    return keys.reshape(H, W)


def shade_stage(keys, sx, sy, zq, ok, zv, color, faces, background):
    """Float64 interpolation and quantisation of one view: perspective-correct barycentrics (lambda_k / z_k, normalised) of the vertex
    colours, floor(255 c + 0.5).  background uint8 [H,W,3].  -> uint8 [H,W,3]."""
    H, W = keys.shape
    out = np.array(background, np.uint8).reshape(H, W, 3).copy()
    cov = keys != EMPTY
    if not cov.any():
        return out
    sx, sy, zq = (np.asarray(a, np.int64) for a in (sx, sy, zq))
    fid = (keys[cov] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    f = np.asarray(faces, np.int64)[fid].copy()
    x, y = sx[f], sy[f]
    area = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])
    f[area < 0] = f[area < 0][:, [0, 2, 1]]
    yy, xx = np.nonzero(cov)
    w, _ = _edges(sx[f], sy[f], xx * 256 + 128, yy * 256 + 128)
    w = np.stack(w, 1).astype(np.float64)
    lam = w / w.sum(1, keepdims=True) / np.asarray(zv, np.float64)[f]
    m = lam / lam.sum(1, keepdims=True)
    c = (m[:, :, None] * np.asarray(color, np.float64)[f]).sum(1)
    out[yy, xx] = np.clip(np.floor(255.0 * c + 0.5), 0, 255).astype(np.uint8)
    return out


def frame_bytes(image_chw):
    """The frame behind the overlay: the batch's float32 image (frame - 0.5) -> floor(255 (image + 0.5) + 0.5) in float32, as the kernel."""
    v = (np.asarray(image_chw, np.float32) + np.float32(0.5)) * np.float32(255.0) + np.float32(0.5)
    return np.clip(np.floor(v), 0, 255).astype(np.uint8).transpose(1, 2, 0)


def draw_sample(hand_verts, hand_faces, K, image_chw, obj=None, vs=None):
    """Panels 2 and 3 of one sample from float inputs.  -> (overlay, free view) uint8 [H,W,3], keys of both, the vertex stage."""
    H, W = image_chw.shape[1:]
    vs = vs or vertex_stage(hand_verts, hand_faces, K, W, H, obj)
    bgs = (frame_bytes(image_chw), np.full((H, W, 3), 255, np.uint8))
    panels, keys = [], []
    for v in (0, 1):
        d = vs[v]
        k = raster_stage(d["sx"], d["sy"], d["zq"], d["ok"], vs["faces"], W, H, vs["nhf"] if v == 0 else None)
        panels.append(shade_stage(k, d["sx"], d["sy"], d["zq"], d["ok"], d["zv"], vs["color"], vs["faces"], bgs[v]))
        keys.append(k)
    return panels[0], panels[1], keys, vs


def exempt_mask(vs, view, keys, W, H, depth_levels):
    """Pixels where float rounding of the vertex stage may legitimately change the outcome, from the oracle alone: the centre is closer
    than 2/256 px to an edge of a triangle that wins there or at a 4-neighbour, or the two nearest fragments differ by less than
    `depth_levels` depth levels."""
    d = vs[view]
    faces = vs["faces"][:vs["nhf"]] if view == 0 else vs["faces"]
    sx, sy = d["sx"].astype(np.float64), d["sy"].astype(np.float64)
    ex = np.zeros((H, W), bool)
    yy, xx = np.mgrid[0:H, 0:W]
    px, py = xx * 256.0 + 128.0, yy * 256.0 + 128.0
    for dy, dx in ((0, 0), (0, 1), (0, -1), (1, 0), (-1, 0)):
        kk = np.full((H, W), EMPTY, np.uint64)
        ys, xs = slice(max(dy, 0), H + min(dy, 0)), slice(max(dx, 0), W + min(dx, 0))
        yd, xd = slice(max(-dy, 0), H + min(-dy, 0)), slice(max(-dx, 0), W + min(-dx, 0))
        kk[yd, xd] = keys[ys, xs]                            # the winner at the neighbour (y + dy, x + dx), looked at from (y, x)
        cov = kk != EMPTY
        f = faces[(kk[cov] & np.uint64(0xFFFFFFFF)).astype(np.int64)]
        for a, b in ((0, 1), (1, 2), (2, 0)):
            ax, ay, bx, by = sx[f[:, a]], sy[f[:, a]], sx[f[:, b]], sy[f[:, b]]
            ln = np.hypot(bx - ax, by - ay)
            dist = np.abs((bx - ax) * (py[cov] - ay) - (by - ay) * (px[cov] - ax)) / np.maximum(ln, 1e-9)
            hit = np.zeros((H, W), bool)
            hit[cov] = dist < 2.0
            ex |= hit
    ex |= second_depth_gap(d, faces, keys, W, H) < depth_levels
    return ex


def second_depth_gap(d, faces, keys, W, H):
    """Per pixel: depth of the second nearest fragment minus depth of the nearest (2^24 where there is no second)."""
    first = (keys >> np.uint64(32)).astype(np.int64)
    fid = np.where(keys != EMPTY, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    faces2 = np.asarray(faces).copy()
    # a second pass without the winners: drop, per pixel, the winning face by rastering all faces and masking it out
    sx, sy, zq, ok = d["sx"], d["sy"], d["zq"], d["ok"]
    gap = np.full((H, W), 1 << 24, np.int64)
    second = _raster_excluding(sx, sy, zq, ok, faces2, W, H, fid)
    has = (second != EMPTY) & (keys != EMPTY)
    gap[has] = (second[has] >> np.uint64(32)).astype(np.int64) - first[has]
    return gap


def _raster_excluding(sx, sy, zq, ok, faces, W, H, fid):
    """raster_stage, but a fragment of face fid[y, x] does not take part at (y, x)."""
    sx, sy, zq = (np.asarray(a, np.int64) for a in (sx, sy, zq))
    keys = np.full(H * W, EMPTY, np.uint64)
    ids, f = _oriented(sx, sy, zq, np.asarray(ok, bool), faces)
    x, y, z = sx[f], sy[f], zq[f]
    x0 = np.maximum(0, (x.min(1) - 128 + 255) >> 8)
    x1 = np.minimum(W - 1, (x.max(1) - 128) >> 8)
    y0 = np.maximum(0, (y.min(1) - 128 + 255) >> 8)
    y1 = np.minimum(H - 1, (y.max(1) - 128) >> 8)
    flat = fid.reshape(-1)
    for i in np.nonzero((x0 <= x1) & (y0 <= y1))[0] if len(ids) else []:
        Y, X = np.mgrid[y0[i]:y1[i] + 1, x0[i]:x1[i] + 1]
        w, bias = _edges(x[i], y[i], X * 256 + 128, Y * 256 + 128)
        cov = (w[0] >= bias[0]) & (w[1] >= bias[1]) & (w[2] >= bias[2]) & (flat[Y * W + X] != ids[i])
        if not cov.any():
            continue
        num = w[0] * z[i, 0] + w[1] * z[i, 1] + w[2] * z[i, 2]
        q = num[cov] // (w[0] + w[1] + w[2])[cov]
        np.minimum.at(keys, (Y * W + X)[cov], (q.astype(np.uint64) << np.uint64(32)) | np.uint64(ids[i]))
    return keys.reshape(H, W)
