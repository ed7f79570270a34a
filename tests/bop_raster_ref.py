"""The stage contract of ab_vsd (include/artiboost_hip.h) restated for the tests, one pixel at a time:
  A  numpy fp32 scalars in the stated order: camera point ((r0 x + r1 y) + r2 z) + t, u = fx (X / Z) + cx, snap floor(u 256 + 0.5); a triangle
     is dropped when a vertex has Z <= NEAR or a snapped coordinate outside +-RANGE, or when its area is zero
  B  python integers: the three edge functions at the pixel sample (x 256, y 256) -- pixel (x, y) is sampled AT (x, y) -- and the top-left rule
  C  numpy float64: l_i = E_i / A, Z = 1 / ((l0 / Z0 + l1 / Z1) + l2 / Z2), rounded to fp32; the nearest surface wins
  D  numpy float64 in the order of bop_toolkit's depth_im_to_dist_im_fast, _estimate_visib_mask (bop19) and vsd (cost_type "step")
`vsd_ref` returns the depth images [B,3,H,W] (est, gt, test), the counts [B,2+T] and the errors [B,T] (float64 and rounded to fp32).
`render_depth` is the renderer the golden script hands to the reference's vsd."""
import numpy as np

F32, F64 = np.float32, np.float64
NEAR = F32(0.01)          # AB_VSD_NEAR, metres
RANGE = 1 << 22           # AB_VSD_RANGE, 1/256 px


def snap_vertices(P, K):
    """Stage A's projection of camera points P [V,3] (fp32) -> [(sx, sy, Z fp32) or None]."""
    fx, cx, fy, cy = F32(K[0]), F32(K[2]), F32(K[4]), F32(K[5])
    out = []
    with np.errstate(all="ignore"):
        for X, Y, Z in np.asarray(P, F32):
            if not Z > NEAR:
                out.append(None)
                continue
            u, v = fx * (X / Z) + cx, fy * (Y / Z) + cy
            su, sv = np.floor(u * F32(256.0) + F32(0.5)), np.floor(v * F32(256.0) + F32(0.5))
            assert su.dtype == F32
            if not (abs(su) <= RANGE and abs(sv) <= RANGE):
                out.append(None)
                continue
            out.append((int(su), int(sv), Z))
    return out


def pose_points(R, t, verts):
    R, t, v = np.asarray(R, F32).reshape(3, 3), np.asarray(t, F32).reshape(3), np.asarray(verts, F32)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    return np.stack([((R[i, 0] * x + R[i, 1] * y) + R[i, 2] * z) + t[i] for i in range(3)], 1)


def _edge(a, b, px, py):
    return (b[0] - a[0]) * (py - a[1]) - (b[1] - a[1]) * (px - a[0])


def _top_left(a, b):
    dx, dy = b[0] - a[0], b[1] - a[1]
    return dy > 0 or (dy == 0 and dx < 0)


def raster(zb, snapped, faces):
    """Stages B and C: `faces` over the snapped vertices into zb [H,W] fp32 (+inf = empty)."""
    H, W = zb.shape
    for ia, ib, ic in np.asarray(faces).reshape(-1, 3).tolist():
        a, b, c = snapped[ia], snapped[ib], snapped[ic]
        if a is None or b is None or c is None:
            continue
        area = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
        if area == 0:
            continue
        if area < 0:
            b, c, area = c, b, -area
        x0, x1 = max(-(-min(a[0], b[0], c[0]) // 256), 0), min(max(a[0], b[0], c[0]) // 256, W - 1)
        y0, y1 = max(-(-min(a[1], b[1], c[1]) // 256), 0), min(max(a[1], b[1], c[1]) // 256, H - 1)
        for y in range(y0, y1 + 1):
            for x in range(x0, x1 + 1):
                px, py = x * 256, y * 256
                e = (_edge(b, c, px, py), _edge(c, a, px, py), _edge(a, b, px, py))
                if min(e) < 0:
                    continue
                if (e[0] == 0 and not _top_left(b, c)) or (e[1] == 0 and not _top_left(c, a)) or (e[2] == 0 and not _top_left(a, b)):
                    continue
                assert e[0] + e[1] + e[2] == area
                A = F64(area)
                l0, l1, l2 = F64(e[0]) / A, F64(e[1]) / A, F64(e[2]) / A
                z = F32(F64(1.0) / ((l0 / F64(a[2]) + l1 / F64(b[2])) + l2 / F64(c[2])))
                if z < zb[y, x]:
                    zb[y, x] = z


def render_depth(verts, faces, R, t, K, W, H):
    """Depth image [H,W] fp32 (0 = nothing) of a mesh under (R, t); verts already in the camera frame when R is None."""
    zb = np.full((H, W), np.inf, F32)
    P = np.asarray(verts, F32) if R is None else pose_points(R, t, verts)
    raster(zb, snap_vertices(P, np.asarray(K, F32).reshape(9)), faces)
    zb[np.isinf(zb)] = 0.0
    return zb


def nearest_positive(*images):
    """Per pixel the smallest value > 0 of the images, 0 where none is."""
    out = np.zeros_like(images[0])
    for im in images:
        take = (im > 0) & ((out == 0) | (im < out))
        out = np.where(take, im, out)
    return out


def stage_d(de, dg, dt, K, delta, taus, diameter, normalized):
    """-> [union, complement, cost per tau] (python ints).  K, delta, taus and diameter are the fp32 values the kernel receives."""
    K = np.asarray(K, F32).reshape(9).astype(F64)
    H, W = de.shape
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    pX, pY = (xs - K[2]) / K[0], (ys - K[5]) / K[4]
    dist = lambda d: np.sqrt((pX * d) ** 2 + (pY * d) ** 2 + d.astype(F64) ** 2)      # noqa: E731
    Le, Lg, Lt = dist(de), dist(dg), dist(dt)
    d32 = F32(delta)
    vis_gt = np.logical_and(np.logical_or(Lg.astype(F32) - Lt.astype(F32) <= d32, Lt == 0), Lg > 0)
    vis_est = np.logical_and(np.logical_or(Le.astype(F32) - Lt.astype(F32) <= d32, Lt == 0), Le > 0)
    vis_est = np.logical_or(vis_est, np.logical_and(vis_gt, Le > 0))
    inter, union = np.logical_and(vis_gt, vis_est), np.logical_or(vis_gt, vis_est)
    dd = np.abs(Lg[inter] - Le[inter])
    if normalized:
        dd = dd / F64(F32(diameter))
    n_union = int(union.sum())
    return [n_union, n_union - int(inter.sum())] + [int((dd >= F64(F32(t))).sum()) for t in taus]


def vsd_ref(meshes, rows, rot_est, tsl_est, rot_gt, tsl_gt, cam_intr, W, H, delta, taus, diameter, normalized=True, depth_test=None, occ_verts=None,
            occ_faces=None):
    """meshes: [(verts, faces)] per table row; diameter: per row.  -> dict depth [B,3,H,W] fp32, counts [B,2+T], err64 [B,T], err [B,T] fp32."""
    B, T = len(rows), len(taus)
    depth, counts, err = np.zeros((B, 3, H, W), F32), np.zeros((B, 2 + T), np.int64), np.ones((B, T), F64)
    for b in range(B):
        v, f = meshes[int(rows[b])]
        K = np.asarray(cam_intr[b], F32).reshape(9)
        de, dg = render_depth(v, f, rot_est[b], tsl_est[b], K, W, H), render_depth(v, f, rot_gt[b], tsl_gt[b], K, W, H)
        dm = np.zeros((H, W), F32) if depth_test is None else np.asarray(depth_test[b], F32)
        dt = dm if occ_verts is None else nearest_positive(render_depth(occ_verts[b], occ_faces, None, None, K, W, H), dg, dm)
        depth[b] = de, dg, dt
        c = stage_d(de, dg, dt, K, delta, taus, diameter[int(rows[b])], normalized)
        counts[b] = c
        if c[0] > 0:
            err[b] = (np.asarray(c[2:], F64) + c[1]) / F64(c[0])
    return dict(depth=depth, counts=counts, err64=err, err=err.astype(F32))
