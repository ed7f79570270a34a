"""Metric plugin classes used on the hot path (anakin/metrics/evaluator.py:12-85, meanepe.py:13-101,
val_metric.py:28-143, lossesmetric.py): Mean3DEPE (MPJPE/MPCPE in mm) and ValMetricMean3DEPE2, whose per-(object,
view, grasp) errors drive the CCV re-weighting (ArtiBoostLoader.step_eval)."""
from typing import Dict, List

import numpy as np
import torch

from .registry import CONST, METRIC, Queries, SynthQueries


class AverageMeter:
    def __init__(self):
        self.reset()

    def reset(self):
        self.avg, self.sum, self.count = 0.0, 0.0, 0

    def update(self, val, n=1):
        self.sum += val
        self.count += n
        self.avg = self.sum / self.count if self.count else 0.0


class Metric:
    def reset(self):
        pass

    def feed(self, preds, targs, **kwargs):
        pass

    def get_measures(self, **kwargs):
        return {}

    # Two-phase feeding (Evaluator.feed_all): `feed_device` enqueues the metric's device arithmetic and returns the small tensors its
    # host bookkeeping needs (None: not deferrable -- the evaluator calls `feed`, which reads the device back at once);
    # `feed_host` receives them as numpy arrays, one step later.  A metric's `feed` is exactly feed_device + feed_host.
    def feed_device(self, preds, targs, **kwargs):
        return None

    def feed_host(self, arrays, **kwargs):
        pass


def _epe_mm(preds, targs, key, mm, memo=None):
    """(B,) mean end-point error of `key`.  memo: per-feed_all cache (several metrics ask for the same key)."""
    if memo is not None:
        mk = ("epe", key, bool(mm))
        if mk not in memo:
            memo[mk] = _epe_mm(preds, targs, key, mm)
        return memo[mk]
    pred = preds[key]
    if "_abs" in key:
        val = targs[key.replace("_abs", "")].to(pred.device) + targs[Queries.ROOT_JOINT].to(pred.device).unsqueeze(1)
    else:
        val = targs[key].to(pred.device)
    diff = pred.detach() - val
    if mm:
        diff = diff * 1000.0
    return torch.norm(diff, p="fro", dim=2).mean(dim=1)       # (B,)


@METRIC.register_module
class Mean3DEPE(Metric):
    def __init__(self, **cfg):
        self.val_keys_list: List[str] = cfg["VAL_KEYS"]
        self.avg_meters = {k: AverageMeter() for k in self.val_keys_list}
        self.to_millimeters = cfg.get("MILLIMETERS", False)
        # meanepe.py:28-31,62-66: --filter_unseen_obj_idxs (through builder.build_evaluator_metric_list(..., arg=arg)) drops the
        # samples of those object classes from the CORNER errors (HO3D's unseen pitcher, README evaluation commands)
        arg = cfg.get("arg", cfg.get("ARG"))
        self.filter_unseen_obj_idxs = list(getattr(arg, "filter_unseen_obj_idxs", []) or []) if arg is not None else []

    def reset(self):
        for m in self.avg_meters.values():
            m.reset()

    def feed_device(self, preds, targs, memo=None, **kwargs):
        """Per key: [sum of the kept samples' errors, number kept] as one (2,) fp32 tensor (no boolean indexing: no host read)."""
        out = []
        for key in self.val_keys_list:
            d = _epe_mm(preds, targs, key, self.to_millimeters, memo)
            n = torch.full((), float(d.shape[0]), dtype=torch.float32, device=d.device)
            if "corners" in key and self.filter_unseen_obj_idxs:
                oi = targs[Queries.OBJ_IDX].to(d.device)
                keep = torch.ones_like(oi, dtype=torch.bool)
                for idx in self.filter_unseen_obj_idxs:
                    keep &= oi != idx
                d = torch.where(keep, d, torch.zeros_like(d))
                n = keep.sum().to(torch.float32)
            out.append(torch.stack([d.sum().to(torch.float32), n]))
        return out

    def feed_host(self, arrays, **kwargs):
        for key, a in zip(self.val_keys_list, arrays):
            self.avg_meters[key].update(float(a[0]), n=int(a[1]))

    def feed(self, preds, targs, **kwargs):
        self.feed_host([t.cpu().numpy() for t in self.feed_device(preds, targs)])

    def get_measures(self, **kwargs):
        return {f"{k}_mepe": m.avg for k, m in self.avg_meters.items()}

    def __str__(self):
        return " | ".join(f"{k}_mepe: {m.avg:6.4f}" for k, m in self.avg_meters.items())


@METRIC.register_module
class ValMetricMean3DEPE2(Metric):
    def __init__(self, **cfg):
        self.val_keys_list: List[str] = cfg["VAL_KEYS"]
        self.storage = {k: {} for k in self.val_keys_list}
        self.to_millimeters = cfg.get("MILLIMETERS", False)

    def reset(self):
        for k in self.storage:
            self.storage[k] = {}

    def feed_device(self, preds, targs, memo=None, **kwargs):
        """[(B, 4) int64 (obj, persp, grasp, is_synth)] + one (B,) error vector per key."""
        d = [_epe_mm(preds, targs, key, self.to_millimeters, memo).to(torch.float32) for key in self.val_keys_list]
        dev = d[0].device if d else None
        ids = torch.stack([torch.as_tensor(targs[k]).to(device=dev, dtype=torch.int64) for k in
                           (SynthQueries.OBJ_ID, SynthQueries.PERSP_ID, SynthQueries.GRASP_ID, SynthQueries.IS_SYNTH)], 1)
        return [ids] + d

    def feed_host(self, arrays, **kwargs):
        ids = arrays[0].tolist()
        for key, d in zip(self.val_keys_list, arrays[1:]):
            st = self.storage[key]
            for i, t in enumerate(ids):
                if t[3]:
                    st[(t[0], t[1], t[2])] = d[i]                          # last write wins (val_metric.py:51-52)

    def feed(self, preds, targs, **kwargs):
        self.feed_host([t.cpu().numpy() for t in self.feed_device(preds, targs)])

    def get_measures(self, **kwargs):
        return dict(self.storage)

    def get_measures_averaged(self, **kwargs) -> Dict:
        stores = [self.storage[k] for k in self.val_keys_list]
        return {k: sum(s[k] for s in stores) / len(stores) for k in stores[0].keys()}

    def __str__(self):
        return ""


@METRIC.register_module
class LossesMetric(Metric):
    def __init__(self, **cfg):
        self.meters = {}

    def reset(self):
        self.meters = {}

    def feed_device(self, preds, targs, losses=None, **kwargs):
        """The step's loss scalars stacked into ONE fp32 vector (the reference reads each with .item(): a host round trip per loss);
        the key order travels on the host side.  Host numbers (python floats) ride along as constants."""
        keys, vals, dev = [], [], None
        for k, v in (losses or {}).items():
            if v is None:
                continue
            keys.append(k)
            vals.append(v)
            if torch.is_tensor(v) and dev is None:
                dev = v.device
        if dev is None:                      # nothing on a device: plain floats
            return [np.asarray([float(v) for v in vals], np.float32)], keys
        return [torch.stack([(v.detach() if torch.is_tensor(v) else torch.as_tensor(float(v))).to(device=dev, dtype=torch.float32).reshape(())
                             for v in vals])], keys

    def feed_host(self, arrays, extra=None, **kwargs):
        for k, v in zip(extra or [], arrays[0].tolist()):
            self.meters.setdefault(k, AverageMeter()).update(v, 1)

    def feed(self, preds, targs, losses=None, **kwargs):
        arrays, keys = self.feed_device(preds, targs, losses=losses)
        self.feed_host([a.cpu().numpy() if torch.is_tensor(a) else a for a in arrays], extra=keys)

    def get_measures(self, **kwargs):
        return {k: m.avg for k, m in self.meters.items()}

    def __str__(self):
        m = self.meters.get("final_loss")
        return f"final_loss: {m.avg:.4e}" if m else ""


class Evaluator:
    """anakin/metrics/evaluator.py:12-85, without a device synchronisation per step.

    The reference's `feed_all` (called after every batch, train_artiboost.py:96-98) moves tensors to the host inside every metric
    (`.item()` per loss scalar, `.cpu()` per error vector): on a GPU that runs ahead of the host each of them stalls the loop until the
    device has drained.  Here a metric with the two-phase API (Metric.feed_device / feed_host: Mean3DEPE, ValMetricMean3DEPE2,
    LossesMetric, the PCK family, ValMetricAR2) only ENQUEUES its arithmetic; the few hundred bytes it needs on the host are packed into
    one pinned buffer with one asynchronous copy + an event, and applied when a later feed_all finds the event complete -- at most `max_lag` steps late (1: the
    progress string of train_artiboost.py:105 shows the numbers through the previous step).  Every read of the measures
    (`metrics_list`, `get_measures_all*`, `dump_images`, `reset_all`) applies what is still in flight first, so at those points the
    state equals per-step blocking feeds exactly.  AR has no host part (its per-object sums stay on the device until they are read);
    the Vis* metrics draw on the host and are fed at once.
    AB_EVAL_BLOCKING=1 (or max_lag=0): every feed applied before feed_all returns."""

    def __init__(self, cfg, metrics_list, max_lag=None):
        import os
        self._metrics_list = metrics_list
        if max_lag is None:
            max_lag = 0 if os.environ.get("AB_EVAL_BLOCKING") == "1" else 1
        self.max_lag = int(max_lag)
        self._inflight = []        # FIFO of (event, pinned buffer, [(metric, [(offset, nbytes, dtype, shape)], extra)])
        self._free = []            # pinned buffers to reuse

    @property
    def metrics_list(self):
        self.flush()               # a reader of the metrics (ArtiBoostLoader.step_eval, the recorder) sees every fed batch
        return self._metrics_list

    def reset_all(self):
        self.flush()
        for m in self._metrics_list:
            m.reset()

    # ---- deferred read-back
    def _apply(self, entry):
        ev, pin, plan = entry
        ev.synchronize()
        host = pin.numpy()
        for m, lay, extra in plan:
            arrays = [host[o:o + nb].view(dt).reshape(shp).copy() for o, nb, dt, shp in lay]
            m.feed_host(arrays, extra=extra)
        self._free.append(pin)

    def _drain(self, keep):
        while len(self._inflight) > keep:
            self._apply(self._inflight.pop(0))
        while self._inflight and self._inflight[0][0].query():      # already on the host: apply (keeps the progress string fresh)
            self._apply(self._inflight.pop(0))

    def flush(self):
        """Apply every feed still in flight (blocks until the device has produced them)."""
        self._drain(0)

    def feed_all(self, preds, targs, losses=None, **kwargs):
        memo, plan, chunks, off = {}, [], [], 0
        dev = None
        for m in self._metrics_list:
            res = m.feed_device(preds, targs, losses=losses, memo=memo) if not isinstance(m, VisMetric) else None
            if res is None:
                m.feed(preds, targs, losses=losses) if isinstance(m, LossesMetric) else m.feed(preds, targs)
                continue
            tensors, extra = res if isinstance(res, tuple) else (res, None)
            if not tensors or not all(torch.is_tensor(t) and t.is_cuda for t in tensors):      # host tensors / numbers / nothing: nothing to wait for
                m.feed_host([t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in tensors], extra=extra)
                continue
            lay = []
            for t in tensors:
                t = t.detach().contiguous()
                dev = t.device
                nb = t.numel() * t.element_size()
                lay.append((off, nb, torch.empty(0, dtype=t.dtype).numpy().dtype, tuple(t.shape)))
                chunks.append(t.view(torch.uint8).reshape(-1) if t.dim() else t.reshape(1).view(torch.uint8))
                pad = (-nb) % 8
                if pad:
                    chunks.append(torch.zeros(pad, dtype=torch.uint8, device=dev))
                off += nb + pad
            plan.append((m, lay, extra))
        if plan:
            blob = torch.cat(chunks) if len(chunks) > 1 else chunks[0]
            pin = None
            for i, b in enumerate(self._free):
                if b.numel() >= off:
                    pin = self._free.pop(i)
                    break
            if pin is None:
                pin = torch.empty(max(off, 4096), dtype=torch.uint8).pin_memory()
            pin[:off].copy_(blob, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(dev))
            self._inflight.append((ev, pin, plan))
        self._drain(self.max_lag)

    def get_measures_all(self):
        self.flush()
        out = {}
        for m in self._metrics_list:
            if isinstance(m, VisMetric):
                continue
            out.update(m.get_measures())
        return out

    def get_measures_all_striped(self, return_losses=True):
        """evaluator.py:58-74: {metric class name: {measure: float}} (scalars only) for the recorder / summarizer."""
        self.flush()
        out = {}
        for m in self._metrics_list:
            if isinstance(m, VisMetric) or (not return_losses and isinstance(m, LossesMetric)):
                continue
            out[type(m).__name__] = {k: float(v) for k, v in m.get_measures().items()
                                     if isinstance(v, (float, int)) or (hasattr(v, "ndim") and getattr(v, "ndim") == 0)}
        return out

    def dump_images(self):
        """evaluator.py:76-82: {metric class name: image} of the Vis* metrics."""
        return {type(m).__name__: m.image for m in self._metrics_list if isinstance(m, VisMetric)}

    def __str__(self):
        """The progress string (train_artiboost.py:105): never waits for the device -- numbers through the last feed already on the host."""
        self._drain(self.max_lag)
        return " | ".join(s for s in (str(m) for m in self._metrics_list if not isinstance(m, VisMetric)) if s)


class VisMetric(Metric):
    """anakin/metrics/vismetric.py:18-68: a metric whose product is an image (skipped by the evaluator's measure tables)."""

    def __init__(self, **cfg):
        self.image, self.count = None, 0

    def reset(self):
        self.count = 0

    def get_measures(self, **kwargs):
        raise NotImplementedError()

    def __str__(self):
        return ""


@METRIC.register_module
class Vis2DMetric(VisMetric):
    """anakin/metrics/vismetric.py:71-200: the first batch fed after a reset is drawn as an NROW x NCOL grid of crops with the
    hand skeleton, the object's box edges, the ground-truth root (star) and box corners 0 / 7 (triangles) -- predictions on the
    left half, ground truth on the right.  `image`: uint8 BGR [H, 2W, 3] like the reference's.  Drawn with PIL (the reference
    uses matplotlib); later batches of the epoch only count."""
    FINGER_COLORS = [(255, 0, 0), (255, 0, 255), (0, 0, 255), (0, 255, 255), (0, 255, 0)]       # thumb .. little (RGB)
    BOX_EDGES = [(0, 1), (1, 3), (3, 2), (2, 0), (4, 5), (5, 7), (7, 6), (6, 4), (1, 5), (2, 6), (3, 7), (0, 4)]

    def __init__(self, **cfg):
        super().__init__(**cfg)
        self.inp_res = cfg["DATA_PRESET"]["IMAGE_SIZE"]
        self.ncol, self.nrow = int(cfg.get("NCOL", 3)), int(cfg.get("NROW", 3))
        self.corner_link_order = list(cfg.get("CORNER_LINK_ORDER", range(8)))

    @staticmethod
    def _images(targs):
        img = targs.get(Queries.IMAGE)
        if img is not None:
            return (img.detach().float().cpu().permute(0, 2, 3, 1) + 0.5).clamp(0, 1).numpy()
        pad = targs["image_nhwc4_padded"]                    # the HIP loader's batch: zero-bordered NHWC4 (fp32 / bf16 or its planes)
        if pad.dim() == 5:
            pad = pad[0].float() + pad[1].float()
        from .registry import image_plane_of
        u8n = image_plane_of(targs, pad) == "u8n"            # the loaders' tag: the integer plane 2 v - 255 (AB_DT_U8N)
        pad = pad.detach().float().cpu()
        if u8n:
            pad = pad / 510.0
        return (pad[:, 3:-3, 3:-5, :3] + 0.5).clamp(0, 1).numpy()

    def _draw(self, images, joints, corners, root, jvis, cvis):
        from PIL import Image, ImageDraw
        W, H = int(self.inp_res[0]), int(self.inp_res[1])
        grid = Image.new("RGB", (self.ncol * W, self.nrow * H))
        for i in range(min(self.ncol * self.nrow, images.shape[0])):
            tile = Image.fromarray((images[i] * 255.0 + 0.5).astype(np.uint8)).resize((W, H))
            d = ImageDraw.Draw(tile)
            j, c = joints[i], corners[i]
            for k in range(1, CONST.NUM_JOINTS):
                par = CONST.JOINTS_IDX_PARENTS[k]
                d.line([tuple(j[par]), tuple(j[k])], fill=self.FINGER_COLORS[(k - 1) // 4], width=2)
            for k in range(CONST.NUM_JOINTS):
                r = 2 if jvis is None or jvis[i][k] > 0 else 1
                d.ellipse([j[k][0] - r, j[k][1] - r, j[k][0] + r, j[k][1] + r], outline=(255, 255, 255))
            for a, b in self.BOX_EDGES:
                a, b = self.corner_link_order[a], self.corner_link_order[b]
                d.line([tuple(c[a]), tuple(c[b])], fill=(64, 224, 208), width=2)
            d.regular_polygon((float(root[i][0]), float(root[i][1]), 5), 5, fill=(138, 43, 226))
            d.regular_polygon((float(c[0][0]), float(c[0][1]), 4), 3, fill=(255, 0, 0))
            d.regular_polygon((float(c[7][0]), float(c[7][1]), 4), 3, fill=(255, 255, 0))
            grid.paste(tile, ((i % self.ncol) * W, (i // self.ncol) * H))
        return np.asarray(grid)[:, :, ::-1]

    def feed(self, preds, targs, **kwargs):
        bs = int(targs[Queries.JOINTS_2D].shape[0])
        if self.count > 0:
            self.count += bs
            return
        res = np.asarray(self.inp_res, dtype=np.float32)
        if "2d_uvd" in preds:
            uvd = preds["2d_uvd"].detach().float().cpu().numpy()
            pj, pc = uvd[:, :CONST.NUM_JOINTS, :2] * res, uvd[:, CONST.NUM_JOINTS:CONST.NUM_JOINTS + 8, :2] * res
        else:
            pj, pc = preds["joints_2d"].detach().float().cpu().numpy(), preds["corners_2d"].detach().float().cpu().numpy()
        gj = targs[Queries.JOINTS_2D][:, :CONST.NUM_JOINTS].detach().float().cpu().numpy()
        gc = targs[Queries.CORNERS_2D].detach().float().cpu().numpy()
        jv = targs[Queries.JOINTS_VIS].detach().float().cpu().numpy() if Queries.JOINTS_VIS in targs else None
        cv = targs[Queries.CORNERS_VIS].detach().float().cpu().numpy() if Queries.CORNERS_VIS in targs else None
        images = self._images(targs)
        self.image = np.concatenate([self._draw(images, pj, pc, gj[:, 0], jv, cv), self._draw(images, gj, gc, gj[:, 0], jv, cv)], axis=1)
        self.count += bs


@METRIC.register_module
class VisHand2DMetric(Vis2DMetric):
    """vismetric.py:361: the hand-only variant shares the drawing."""


# ============================================================================ eval / submit path
@METRIC.register_module
class Mean2DEPE(Mean3DEPE):
    """anakin/metrics/meanepe.py:97-101: pixel errors, never scaled to millimetres."""

    def __init__(self, **cfg):
        super().__init__(**cfg)
        self.to_millimeters = False


class PCKMetric(Metric):
    """anakin/metrics/pckmetric.py:12-143: per-keypoint Euclidean errors of the visible keypoints; mean EPE, PCK curve
    over STEPS thresholds in [VAL_MIN, VAL_MAX], AUC by the trapezoid rule normalised by the area under 1."""
    num_kp = 0
    keys = ("", "", "")

    def __init__(self, **cfg):
        self.val_min, self.val_max, self.steps = cfg["VAL_MIN"], cfg["VAL_MAX"], cfg["STEPS"]
        self.reset()

    def reset(self):
        self.data = [[] for _ in range(self.num_kp)]
        self.count = 0

    def feed_device(self, preds, targs, **kwargs):
        """[(B, N) distances (fp32 for fp32 predictions), (B, N) uint8 visibility], both on the predictions' device: nothing is read back."""
        kp, kt, kv = self.keys
        p, t = preds[kp].detach(), targs[kt].to(preds[kp].device)
        dist = torch.sqrt(torch.sum((p - t) ** 2, dim=-1))                          # (B, N)
        vis = (torch.as_tensor(targs[kv]).detach().to(dist.device) != 0).to(torch.uint8)
        assert dist.dim() == 2 and vis.shape == dist.shape
        return [dist, vis]

    def feed_host(self, arrays, **kwargs):
        dist, vis = arrays[0], arrays[1].astype(bool)
        for i in range(self.num_kp):
            self.data[i].extend(dist[vis[:, i], i].tolist())
        self.count += dist.shape[0]

    def feed(self, preds, targs, **kwargs):
        self.feed_host([t.cpu().numpy() for t in self.feed_device(preds, targs)])

    def _get_pck(self, kp_id, threshold):
        if not self.data[kp_id]:
            return None
        return float(np.mean((np.array(self.data[kp_id]) <= threshold).astype("float")))

    def get_pck_all(self, threshold):
        vals = [v for v in (self._get_pck(i, threshold) for i in range(self.num_kp)) if v is not None]
        return float(np.mean(np.array(vals))) if vals else float("nan")

    def get_measures(self, **kwargs):
        thresholds = np.array(np.linspace(self.val_min, self.val_max, self.steps))
        area_under_one = np.trapezoid(np.ones_like(thresholds), thresholds)
        epe, auc, curves = [], [], []
        for i in range(self.num_kp):
            if not self.data[i]:
                continue
            d = np.array(self.data[i])
            epe.append(np.mean(d))
            curve = np.array([np.mean((d <= t).astype("float")) for t in thresholds])
            curves.append(curve)
            auc.append(np.trapezoid(curve, thresholds) / area_under_one)
        return {"epe_mean_per_kp": np.array(epe), "pck_curve_per_kp": np.array(curves), "auc_per_kp": np.array(auc),
                "epe_mean_all": np.mean(np.array(epe)), "auc_all": np.mean(np.array(auc)), "thresholds": thresholds}


def _pck(name, n, keys, label=None):
    def __str__(self):
        return f"{label}: {self.get_pck_all(0.02):6.4f}" if label else ""
    return METRIC.register_module(type(name, (PCKMetric,), {"num_kp": n, "keys": keys, "__str__": __str__,
                                                          "__doc__": "anakin/metrics/pckmetric.py:146-197"}))


Hand3DPCKMetric = _pck("Hand3DPCKMetric", 21, ("joints_3d", "joints_3d", "joints_vis"), "hand3d pck")
Hand2DPCKMetric = _pck("Hand2DPCKMetric", 21, ("joints_2d", "joints_2d", "joints_vis"))
Obj3DPCKMetric = _pck("Obj3DPCKMetric", 8, ("corners_3d", "corners_3d", "corners_vis"), "obj3d pck")
Obj2DPCKMetric = _pck("Obj2DPCKMetric", 8, ("corners_2d", "corners_2d", "corners_vis"))


class _MSSDBase:
    """Maximum symmetry-aware surface distance (anakin/metrics/bopAR.py:74-195, val_metric.py:235-327): per sample
    min over the object's symmetry set of max over the model points of ||sym(gt) - pred||.  The reference loops over the
    object classes with boolean masks (a device synchronisation per class); here the whole batch is one call.

    Each object keeps its OWN set, as in the reference: BOP's get_symmetry_transformations enumerates the discretised continuous
    rotations from i = 1, so the set of an object with a continuous symmetry does NOT contain the identity, and a perfect
    prediction of such an object scores the distance to its nearest listed rotation, not 0.  The table [n_obj, Kmax] is padded by
    repeating a row's FIRST transform (the minimum over the row is unchanged, exactly); `sym_count` holds the true lengths.
    USE_HO3D_YCB: ext (S.R (ext x) + S.t) = (ext S.R ext) x + ext S.t and ext only flips signs, so it is folded into the table once.

    HIP tensors: kernels.mssd (csrc/mssd.hip) -- rigid mode for vertices, points mode for corners, the centre offset when configured;
    it reads only the first `sym_count` entries of a row and builds no [B, K, V, 3] temporary.  AB_MSSD_TORCH=1 keeps the torch
    expression there; CPU tensors always take it."""

    def __init__(self, **cfg):
        import json
        from .criterions import get_symmetry_transformations
        info = cfg.get("MODEL_INFO") or json.load(open(cfg["MODEL_INFO_PATH"], "r"))
        step = cfg.get("MAX_SYM_DISC_STEP", 0.01)
        self.n_obj = len(info)
        self.mssd_use_corners = cfg.get("MSSD_USE_CORNERS", False)
        self.use_ho3d_ycb = cfg.get("USE_HO3D_YCB", False)
        self.center_idx = cfg["DATA_PRESET"]["CENTER_IDX"] if cfg.get("MSSD_USE_CENTER_IDX", False) else None
        syms = [get_symmetry_transformations(info[str(i)], step) for i in range(1, self.n_obj + 1)]
        kmax = max(len(x) for x in syms)
        R = np.zeros((self.n_obj, kmax, 3, 3))
        t = np.zeros((self.n_obj, kmax, 3, 1))
        ext = np.diag([1.0, -1.0, -1.0]) if self.use_ho3d_ycb else np.eye(3)
        for i, tr in enumerate(syms):
            for k in range(kmax):
                x = tr[k] if k < len(tr) else tr[0]
                R[i, k], t[i, k] = ext @ x["R"] @ ext, ext @ x["t"]
        self.R, self.t = torch.Tensor(R), torch.Tensor(t) / 1000.0                 # mm -> m
        self.sym_count = torch.tensor([len(x) for x in syms], dtype=torch.int32)
        self._dev = None

    def values(self, preds, targs):
        """-> (obj_idx [B] int64 1-based, mssd [B] in metres), both on the predictions' device."""
        import os
        dev = preds["box_rot_rotmat"].device
        if self._dev != dev:
            self.R, self.t, self.sym_count, self._dev = self.R.to(dev), self.t.to(dev), self.sym_count.to(dev), dev
        can = targs[Queries.CORNERS_CAN if self.mssd_use_corners else "obj_verts_can"].to(dev)
        transf = targs[Queries.OBJ_TRANSF].to(dev)
        obj_idx = targs[Queries.OBJ_IDX].to(dev).long()
        center = None
        if self.center_idx is not None:
            center = targs[Queries.ROOT_JOINT].to(dev) - preds["joints_3d_abs"][:, self.center_idx].detach()
        if dev.type == "cuda" and os.environ.get("AB_MSSD_TORCH") != "1":
            from . import kernels as K
            f = lambda x: None if x is None else x.detach().to(torch.float32).contiguous()      # noqa: E731
            if self.mssd_use_corners:
                mode = dict(pred_pts=f(preds["corners_3d_abs"]))
            else:
                mode = dict(pred_R=f(preds["box_rot_rotmat"]), pred_t=f(preds["boxroot_3d_abs"]))
            return obj_idx, K.mssd(f(can), f(transf), obj_idx.contiguous(), self.R, self.t, self.sym_count, center=f(center), **mode)
        sym_R, sym_t = self.R[obj_idx - 1], self.t[obj_idx - 1]                      # [B,K,3,3], [B,K,3,1]
        sym_can = (torch.einsum("bkmn,bvn->bkmv", sym_R, can) + sym_t).transpose(-2, -1)
        sym_abs = (torch.einsum("bij,bklj->bkil", transf[:, :3, :3], sym_can) + transf[:, None, :3, 3:]).transpose(-2, -1)
        if self.mssd_use_corners:
            pred_abs = preds["corners_3d_abs"]
        else:
            pred_abs = (preds["box_rot_rotmat"] @ can.transpose(-2, -1)).transpose(-2, -1) + preds["boxroot_3d_abs"]
        if center is None:
            d = sym_abs - pred_abs.unsqueeze(1)
        else:
            d = ((sym_abs - targs[Queries.ROOT_JOINT].to(dev)[:, None, None, :]) -
                 (pred_abs - preds["joints_3d_abs"][:, [self.center_idx]]).unsqueeze(1))
        return obj_idx, torch.norm(d, dim=-1).max(-1)[0].min(-1)[0].detach()


@METRIC.register_module
class AR(Metric):
    """anakin/metrics/bopAR.py:15-61 with USE_MSSD: a mean MSSD in millimetres.  USE_VSD / USE_MSPD raise NotImplementedError, as in the
    reference, whose VSD and MSPD are stubs; the BOP average recall over VSD, MSSD and MSPD is the metric type BOPRecall (below)."""

    def __init__(self, **cfg):
        if cfg.get("USE_VSD", False) or cfg.get("USE_MSPD", False):
            raise NotImplementedError()
        self.mssd = _MSSDBase(**cfg) if cfg.get("USE_MSSD", False) else None
        self.reset()

    def reset(self):
        self._sum = self._cnt = None

    def feed(self, preds, targs, **kwargs):
        if self.mssd is None:
            return
        obj_idx, v = self.mssd.values(preds, targs)
        if self._sum is None:
            self._sum = torch.zeros(self.mssd.n_obj, dtype=torch.float64, device=v.device)
            self._cnt = torch.zeros(self.mssd.n_obj, dtype=torch.float64, device=v.device)
        self._sum.index_add_(0, obj_idx - 1, v.double())                 # per-object sums stay on the device: no sync per step
        self._cnt.index_add_(0, obj_idx - 1, torch.ones_like(v, dtype=torch.float64))

    @property
    def objs_error(self):
        out = {i + 1: AverageMeter() for i in range(self.mssd.n_obj)}
        if self._sum is not None:
            for i, (s_, c_) in enumerate(zip(self._sum.cpu().tolist(), self._cnt.cpu().tolist())):
                if c_:
                    out[i + 1].update(s_, n=int(c_))
        return out

    @property
    def avg(self):
        if self._sum is None:
            return float("nan")
        c = float(self._cnt.sum())
        return float(self._sum.sum()) / c * 1000.0 if c else float("nan")

    def get_measures(self, **kwargs):
        if self.mssd is None:
            return {}
        tag = ".corner" if self.mssd.mssd_use_corners else ""
        out = {"MSSD": self.avg}
        out.update({f"{i}{tag}.mssd": m.avg * 1000.0 for i, m in self.objs_error.items()})
        return out

    def __str__(self):
        return f"mssd: {self.avg:6.4f}" if self.mssd is not None else ""


@METRIC.register_module
class ValMetricAR2(Metric):
    """anakin/metrics/val_metric.py:145-222: per-(object, view, grasp) MSSD in mm of the synthetic samples (last write
    wins), the second mining signal ArtiBoostLoader.get_evaluator_result accepts (artiboost_loader.py:301-327)."""

    def __init__(self, **cfg):
        if cfg.get("USE_VSD", False) or cfg.get("USE_MSPD", False):
            raise NotImplementedError()
        self.mssd = _MSSDBase(**cfg) if cfg.get("USE_MSSD", False) else None
        self.reset()

    def reset(self):
        self.storage = {}

    def feed_device(self, preds, targs, **kwargs):
        """[(B, 4) int64 (obj_id, persp_id, grasp_id, is_synth), (B,) int64 obj_idx, (B,) fp32 MSSD in mm] on the predictions' device."""
        if self.mssd is None:
            return None
        obj_idx, v = self.mssd.values(preds, targs)
        ids = torch.stack([torch.as_tensor(targs[k]).to(device=v.device, dtype=torch.int64) for k in
                           (SynthQueries.OBJ_ID, SynthQueries.PERSP_ID, SynthQueries.GRASP_ID, SynthQueries.IS_SYNTH)], 1)
        return [ids, obj_idx, (v * 1000.0).to(torch.float32)]

    def feed_host(self, arrays, **kwargs):
        ids, obj_idx, vals = arrays[0].tolist(), arrays[1], arrays[2]
        for i in np.argsort(obj_idx, kind="stable"):                     # the reference visits the object classes in order:
            t = ids[i]                                                   # later classes overwrite earlier ones on a repeated triplet
            if t[3]:
                self.storage[(t[0], t[1], t[2])] = vals[i]

    def feed(self, preds, targs, **kwargs):
        res = self.feed_device(preds, targs)
        if res is not None:
            self.feed_host([t.cpu().numpy() for t in res])

    def get_measures(self, **kwargs):
        return {"mssd": self.storage} if self.mssd is not None else {}

    def get_measures_averaged(self, **kwargs):
        return dict(self.storage)

    def __str__(self):
        return ""


# ============================================================================ leaderboard mesh metrics
MESH_F_THRESHOLDS_MM = (5.0, 15.0)       # the thresholds HO3D / FreiHAND publish F-scores at


def mesh_values_torch(pred, targ, root=None, center_idx=-1, thresholds=(), flags=7, want_dist=False):
    """The definitions of ab_mesh_metrics (include/artiboost_hip.h) as torch ops, in the tensors' dtype: the route of CPU tensors, and what
    tools/bench_mesh_metrics.py times on device tensors.  Same arguments and the same dict as kernels.mesh_metrics: rows [B,16] (columns
    kernels.MM_ROW, NaN where a group was not asked for), counts int32 [B,T,4] and, with want_dist, the four per-point distance arrays.
    The nearest-neighbour scan is one [N,M] matrix of squared direct differences per sample (not torch.cdist: on the HIP build this project
    runs on, its batched no-matmul form returned distances 0.2 m off for every sample but the first at B = 64, N = M = 778; DESIGN.md
    section 23)."""
    from .kernels import MM_NN, MM_PAIRED, MM_PROCRUSTES, MM_ROW as C
    P = pred.detach()
    G = targ.to(P.device) if root is None else targ.to(P.device) + root.to(P.device).unsqueeze(1)
    B, N, M, T = P.shape[0], P.shape[1], G.shape[1], len(thresholds)
    if flags & (MM_PAIRED | MM_PROCRUSTES) and N != M:
        raise ValueError(f"mesh_values_torch: paired and aligned errors need N == M, got {N} and {M}")
    if flags & MM_PROCRUSTES and N < 3:
        raise ValueError("mesh_values_torch: the alignment needs N >= 3")
    rows = torch.full((B, 16), float("nan"), dtype=P.dtype, device=P.device)
    counts = torch.zeros((B, T, 4), dtype=torch.int32, device=P.device)
    out = {"rows": rows, "counts": counts}
    if flags & MM_PAIRED:
        rows[:, C["epe"]] = torch.norm(P - G, dim=2).mean(1)
        if center_idx >= 0:
            c = slice(center_idx, center_idx + 1)
            rows[:, C["ra_epe"]] = torch.norm((P - P[:, c]) - (G - G[:, c]), dim=2).mean(1)
    Pa = None
    if flags & MM_PROCRUSTES:         # AlignLoss.procrustes_align, keeping the scale: R = u v^T of Gh^T Ph, no determinant correction
        mg, mp = G.mean(1, keepdim=True), P.mean(1, keepdim=True)
        c = torch.norm(G - mg, dim=(1, 2), keepdim=True) + 1e-8
        p = torch.norm(P - mp, dim=(1, 2), keepdim=True) + 1e-8
        Ph = (P - mp) / p
        u, w, vh = torch.linalg.svd(((G - mg) / c).transpose(1, 2) @ Ph)
        s = w.sum(1).reshape(B, 1, 1)
        Pa = (Ph @ (u @ vh).transpose(1, 2)) * (s * c) + mg
        rows[:, C["pa_epe"]] = torch.norm(Pa - G, dim=2).mean(1)
        rows[:, C["scale"]] = (s * c / p).reshape(B)
    if flags & MM_NN:
        thr = torch.as_tensor([float(t) for t in thresholds], dtype=P.dtype, device=P.device)
        for k, (Q, pre) in enumerate(((P, ""), (Pa, "pa_"))):
            if Q is None:
                continue
            d_pg, d_gp = [], []
            for qb, gb in zip(Q, G):      # one sample at a time, as criterions.chamfer_distance_torch: one [N,M] matrix of direct differences
                d2 = ((qb[:, None, :] - gb[None, :, :]) ** 2).sum(-1)
                d_pg.append(d2.min(1)[0]); d_gp.append(d2.min(0)[0])
            d_pg, d_gp = torch.stack(d_pg).sqrt(), torch.stack(d_gp).sqrt()
            rows[:, C[pre + "mean_pg"]], rows[:, C[pre + "mean_gp"]] = d_pg.mean(1), d_gp.mean(1)
            if T:
                n_pg, n_gp = (d_pg.unsqueeze(1) < thr[None, :, None]).sum(2), (d_gp.unsqueeze(1) < thr[None, :, None]).sum(2)   # [B,T], strict <
                counts[:, :, 2 * k], counts[:, :, 2 * k + 1] = n_pg.to(torch.int32), n_gp.to(torch.int32)
                pr, rc = n_pg.to(P.dtype) / N, n_gp.to(P.dtype) / M
                rows[:, C[pre + "f"]:C[pre + "f"] + T] = torch.where(pr + rc > 0, 2 * pr * rc / (pr + rc).clamp_min(1e-30), torch.zeros_like(pr))
            if want_dist:
                out[pre + "d_pg"], out[pre + "d_gp"] = d_pg, d_gp
    return out


def _mesh_values(preds, targs, key, memo=None, center_idx=-1, thresholds=None):
    """rows / counts (the dict of kernels.mesh_metrics) of `key`, or None when the batch lacks the prediction or its target.  ONE call per
    key per feed_all: every mesh metric asks for the same thing -- all the groups the shapes allow (N == M >= 3: paired, aligned and
    nearest-neighbour; otherwise nearest-neighbour only), the centre on 21-joint arrays only, thresholds None = the published 5 / 15 mm --
    so the `memo` of Evaluator.feed_all serves the second and third metric over a key.  Keys resolve as in _epe_mm: a `*_abs` key is
    compared against targs[key without _abs] + root_joint.  HIP tensors: ab_mesh_metrics; CPU tensors: mesh_values_torch."""
    thr = tuple(float(t) for t in (thresholds if thresholds is not None else [t / 1000.0 for t in MESH_F_THRESHOLDS_MM]))
    tkey = key.replace("_abs", "") if "_abs" in key else key
    if preds.get(key) is None or targs.get(tkey) is None or ("_abs" in key and targs.get(Queries.ROOT_JOINT) is None):
        return None
    pred = preds[key].detach()
    N, M = pred.shape[1], targs[tkey].shape[1]
    center = int(center_idx) if N == CONST.NUM_JOINTS and N == M else -1
    mk = ("mesh", key, center, thr)
    if memo is not None and mk in memo:
        return memo[mk]
    from . import kernels as K
    flags = (K.MM_PAIRED | K.MM_PROCRUSTES | K.MM_NN) if N == M and N >= 3 else K.MM_NN
    f = lambda t: t.to(device=pred.device, dtype=torch.float32).contiguous()      # noqa: E731
    root = f(targs[Queries.ROOT_JOINT]) if "_abs" in key else None
    fn = K.mesh_metrics if pred.is_cuda else mesh_values_torch
    val = dict(fn(f(pred), f(targs[tkey]), root, center_idx=center, thresholds=thr, flags=flags), n_points=(N, M))
    if memo is not None:
        memo[mk] = val
    return val


class _MeshMetric(Metric):
    """Shared bookkeeping of the three mesh metrics: per measure one [sum over samples, count] pair from feed_device (nothing there reads
    the device), averaged over samples on the host -- the mean over samples of the per-sample value, as the scoring scripts average.
    A key whose prediction or target a batch lacks is skipped for that batch and logged once (HO3D's evaluation split has no hand
    annotation).  --filter_unseen_obj_idxs is NOT honoured by these classes."""

    def __init__(self, **cfg):
        self.val_keys_list: List[str] = list(cfg["VAL_KEYS"])
        self.to_millimeters = cfg.get("MILLIMETERS", False)
        self.center_idx = int(cfg.get("CENTER_IDX", (cfg.get("DATA_PRESET") or {}).get("CENTER_IDX", 0)))
        self.thresholds = None
        self.avg_meters: Dict[str, AverageMeter] = {}
        self._skipped = set()

    def reset(self):
        for m in self.avg_meters.values():
            m.reset()

    def _measures(self, key, val):
        """[(measure name, (B,) tensor)] of one key."""
        raise NotImplementedError()

    def _col(self, val, name, k=0):
        from .kernels import MM_ROW
        d = val["rows"][:, MM_ROW[name] + k]
        return d * 1000.0 if self.to_millimeters and name not in ("f", "pa_f") else d

    def feed_device(self, preds, targs, memo=None, **kwargs):
        names, out = [], []
        for key in self.val_keys_list:
            val = _mesh_values(preds, targs, key, memo, self.center_idx, self.thresholds)
            if val is None:
                if key not in self._skipped:
                    self._skipped.add(key)
                    import logging
                    logging.getLogger("anakin").warning(f"{type(self).__name__}: batch without '{key}' or its target; the key is skipped for such batches")
                continue
            for name, d in self._measures(key, val):
                n = torch.full((), float(d.shape[0]), dtype=torch.float32, device=d.device)
                names.append(name)
                out.append(torch.stack([d.sum().to(torch.float32), n]))
        return out, names

    def feed_host(self, arrays, extra=None, **kwargs):
        for name, a in zip(extra or [], arrays):
            self.avg_meters.setdefault(name, AverageMeter()).update(float(a[0]), n=int(a[1]))

    def feed(self, preds, targs, **kwargs):
        out, names = self.feed_device(preds, targs)
        self.feed_host([t.cpu().numpy() for t in out], extra=names)

    def get_measures(self, **kwargs):
        return {k: m.avg for k, m in self.avg_meters.items()}

    def __str__(self):
        return " | ".join(f"{k}: {m.avg:6.4f}" for k, m in self.avg_meters.items())


@METRIC.register_module
class MeanAlignedEPE(_MeshMetric):
    """PA-MPJPE / PA-MPVPE and the root-relative error: `{key}_pa_mepe` (after the similarity alignment of the prediction onto the target:
    rotation or reflection, scale, translation) and `{key}_ra_mepe` (both clouds relative to their CENTER_IDX point).  ALIGN: a subset of
    {root, procrustes}, default [procrustes]; `root` is defined for 21-joint arrays only.  CENTER_IDX defaults to DATA_PRESET.CENTER_IDX."""

    def __init__(self, **cfg):
        super().__init__(**cfg)
        self.align = list(cfg.get("ALIGN", ["procrustes"]))
        if not self.align or set(self.align) - {"root", "procrustes"}:
            raise ValueError(f"MeanAlignedEPE: ALIGN must be a non-empty subset of [root, procrustes], got {self.align}")

    def _measures(self, key, val):
        out = []
        N = val["n_points"]
        if N[0] != N[1] or N[0] < 3:
            raise ValueError(f"MeanAlignedEPE: '{key}' pairs {N[0]} predicted with {N[1]} target points; an aligned error needs N == M >= 3")
        if "procrustes" in self.align:
            out.append((f"{key}_pa_mepe", self._col(val, "pa_epe")))
        if "root" in self.align:
            if N[0] != CONST.NUM_JOINTS:
                raise ValueError(f"MeanAlignedEPE: ALIGN root needs a {CONST.NUM_JOINTS}-joint array, '{key}' has {N[0]} points")
            out.append((f"{key}_ra_mepe", self._col(val, "ra_epe")))
        return out


@METRIC.register_module
class MeshFScore(_MeshMetric):
    """Mesh F-scores: per sample the harmonic mean of precision #{d_pg < t} / N and recall #{d_gp < t} / M over the two-way nearest
    distances, `{key}_f{t}` unaligned and `{key}_pa_f{t}` after the similarity alignment (t in mm, printed with %g: f5, f15).
    THRESHOLDS_MM default [5, 15] (at most 4); ALIGN: a subset of {none, procrustes}, default both."""

    def __init__(self, **cfg):
        super().__init__(**cfg)
        self.thresholds_mm = [float(t) for t in cfg.get("THRESHOLDS_MM", MESH_F_THRESHOLDS_MM)]
        self.align = list(cfg.get("ALIGN", ["none", "procrustes"]))
        if not self.align or set(self.align) - {"none", "procrustes"}:
            raise ValueError(f"MeshFScore: ALIGN must be a non-empty subset of [none, procrustes], got {self.align}")
        if not 1 <= len(self.thresholds_mm) <= 4:
            raise ValueError(f"MeshFScore: 1 to 4 THRESHOLDS_MM, got {self.thresholds_mm}")
        self.thresholds = [t / 1000.0 for t in self.thresholds_mm]

    def _measures(self, key, val):
        out = []
        N = val["n_points"]
        if "procrustes" in self.align and (N[0] != N[1] or N[0] < 3):
            raise ValueError(f"MeshFScore: '{key}' pairs {N[0]} predicted with {N[1]} target points; ALIGN procrustes needs N == M >= 3")
        for pre, col in (("none", "f"), ("procrustes", "pa_f")):
            if pre in self.align:
                out += [(f"{key}_{col}{t:g}", self._col(val, col, k)) for k, t in enumerate(self.thresholds_mm)]
        return out


@METRIC.register_module
class MeanSurfaceDist(_MeshMetric):
    """ADD-S of an object mesh: `{key}_adds`, the mean over the points of the posed ground-truth model of the distance to the nearest
    predicted point, unaligned; the two clouds need not have the same number of points."""

    def _measures(self, key, val):
        return [(f"{key}_adds", self._col(val, "mean_gp"))]


# ============================================================================ hand-object interaction
def drop_repeated_faces(faces):
    """The faces whose three indices differ (the stand-in hand pads to 1 538 faces with fans that repeat an index)."""
    f = np.asarray(faces).reshape(-1, 3)
    return np.ascontiguousarray(f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])]).astype(np.int32)


def mesh_orientation(verts, faces):
    """o = sign(sum_f a . (b x c)) in float64: the sign of the mesh's signed volume (+1 for a mesh without volume)."""
    v, f = np.asarray(verts, np.float64), np.asarray(faces).reshape(-1, 3)
    vol = np.einsum("ij,ij->", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]]))
    return -1.0 if vol < 0 else 1.0


def _triangle_scan(q, tri, want_dist, want_cp=False, medial=None):
    """q [Q,3] against tri [F,3,3] as [Q,F] blocks (at most 2^20 pairs at a time) -> (w [Q] = sum_f Omega_f / (4 pi), the smallest squared
    distance [Q] or None), by the definitions of ab_interaction in the tensors' dtype.  want_cp (with want_dist): a third value, the dict
    {r [Q,3]: cp - q of the first face in face order that attains the minimum (through gather), face [Q]: its index} and, with
    medial = (tol_d, tol_cp), also `medial` [Q]: whether a face whose distance is within tol_d of the smallest has its closest point more
    than tol_cp away from the winner's (the query sits near the medial axis: the closest point is not stable under rounding)."""
    import math
    Q, F = q.shape[0], tri.shape[0]
    e1, e2 = (tri[:, 1] - tri[:, 0])[None], (tri[:, 2] - tri[:, 0])[None]
    dot = lambda x, y: (x * y).sum(-1)      # noqa: E731
    ws, ds = [], []
    rs, fs, ms = [], [], []
    step = max(1, (1 << 20) // max(F, 1))
    for s in range(0, Q, step):
        qq = q[s:s + step, None]
        A, B, C = tri[None, :, 0] - qq, tri[None, :, 1] - qq, tri[None, :, 2] - qq
        la, lb, lc = dot(A, A).sqrt(), dot(B, B).sqrt(), dot(C, C).sqrt()
        num = dot(A, torch.cross(B, C, dim=-1))
        den = la * lb * lc + dot(A, B) * lc + dot(B, C) * la + dot(C, A) * lb
        om = torch.where((num == 0) & (den == 0), torch.zeros_like(num), 2.0 * torch.atan2(num, den))
        ws.append(om.sum(1) / (4.0 * math.pi))
        if not want_dist:
            continue
        d1, d2, d3, d4, d5, d6 = -dot(e1, A), -dot(e2, A), -dot(e1, B), -dot(e2, B), -dot(e1, C), -dot(e2, C)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        zero, one = torch.zeros_like(va), torch.ones_like(va)
        nv, nw, dn = vb, vc, (va + vb) + vc                                        # interior; then the regions, the first of the list winning last
        for cond, a, b, c in (((va <= 0) & (e43 >= 0) & (e56 >= 0), e56, e43, e43 + e56),       # edge bc
                              ((vb <= 0) & (d2 >= 0) & (d6 <= 0), zero, d2, d2 - d6),           # edge ac
                              ((d6 >= 0) & (d5 <= d6), zero, one, one),                         # vertex c
                              ((vc <= 0) & (d1 >= 0) & (d3 <= 0), d1, zero, d1 - d3),           # edge ab
                              ((d3 >= 0) & (d4 <= d3), one, zero, one),                         # vertex b
                              ((d1 <= 0) & (d2 <= 0), zero, zero, one)):                        # vertex a
            nv, nw, dn = torch.where(cond, a, nv), torch.where(cond, b, nw), torch.where(cond, c, dn)
        ok = dn != 0
        safe = torch.where(ok, dn, one)
        v, w = torch.where(ok, nv / safe, zero), torch.where(ok, nw / safe, zero)  # a zero denominator gives parameter 0
        r = A + v[..., None] * e1 + w[..., None] * e2
        ds.append(dot(r, r).min(1)[0])
        if want_cp:
            dd = dot(r, r)
            j = dd.min(1)[1]                                                       # the first minimum in face order
            rb = r.gather(1, j[:, None, None].expand(-1, 1, 3))[:, 0]
            rs.append(rb); fs.append(j)
            if medial is not None:
                near = dd.sqrt() <= dd.min(1)[0].sqrt()[:, None] + medial[0]
                ms.append((near & (((r - rb[:, None]) ** 2).sum(-1).sqrt() > medial[1])).any(1))
    if want_dist and want_cp:
        cp = {"r": torch.cat(rs), "face": torch.cat(fs)}
        if medial is not None:
            cp["medial"] = torch.cat(ms)
        return torch.cat(ws), torch.cat(ds), cp
    return torch.cat(ws), (torch.cat(ds) if want_dist else None)


def interaction_values_torch(hand_verts, hand_faces, hand_orient, obj_verts, obj_faces, vert_off, face_off, obj_orient, obj_row, rot, tsl,
                             contact_thr=0.005, voxel=0.005, max_voxels=262144, flags=3, want_sdf=False, want_lattice=False):
    """The definitions of ab_interaction (include/artiboost_hip.h) as torch ops in hand_verts' dtype: the route of CPU tensors, in float64
    the reference of the tests, and what tools/bench_interaction.py times on device tensors.  Same arguments and the same dict as
    kernels.interaction: rows [B,8] (columns kernels.IA_ROW; NaN where a group was not asked for), counts int32 [B,4] and, with want_sdf,
    sdf and wind [B,Nh].  Like the kernel it takes a query into the object's canonical frame, q' = R^T (q - t), and scans the canonical
    triangles, one [Q,F] block per sample; the lattice points of the volume are scanned against the object and, those inside it, against
    the hand mesh of the camera frame.  want_lattice (this route only): also `lattice`, per sample None or (points [n,3], o w of the object [n],
    o w of the hand [n], NaN where the point is outside the object and the hand was not scanned)."""
    from .kernels import IA_ROW as C, IA_VERTS, IA_VOLUME
    hv = hand_verts.detach()
    dt, dev = hv.dtype, hv.device
    B, Nh = hv.shape[0], hv.shape[1]
    n_obj = int(obj_orient.numel())
    rows = torch.full((B, 8), float("nan"), dtype=dt, device=dev)
    counts = torch.zeros((B, 4), dtype=torch.int32, device=dev)
    out = {"rows": rows, "counts": counts}
    if want_sdf:
        out["sdf"], out["wind"] = torch.full((B, Nh), float("nan"), dtype=dt, device=dev), torch.full((B, Nh), float("nan"), dtype=dt, device=dev)
    if want_lattice:
        out["lattice"] = [None] * B
    vo, fo = [int(x) for x in vert_off.cpu()], [int(x) for x in face_off.cpu()]
    orow = [min(max(int(r), 0), n_obj - 1) for r in obj_row.cpu()]
    orient = [float(x) for x in obj_orient.cpu()]
    hf = hand_faces.to(dev).long().reshape(-1, 3)
    R_all, t_all = rot.detach().to(device=dev, dtype=dt).reshape(B, 3, 3), tsl.detach().to(device=dev, dtype=dt).reshape(B, 3)
    for b in range(B):
        r = orow[b]
        can = obj_verts[vo[r]:vo[r + 1]].to(device=dev, dtype=dt)
        tri = can[obj_faces[fo[r]:fo[r + 1]].to(dev).long().reshape(-1, 3)]
        R, t = R_all[b], t_all[b]
        if flags & IA_VERTS:
            w, d2 = _triangle_scan((hv[b] - t) @ R, tri, True)
            w, d = orient[r] * w, d2.sqrt()
            inside = w > 0.5
            n_in = inside.sum()
            din = torch.where(inside, d, torch.zeros_like(d))
            rows[b, C["pen_max"]], rows[b, C["pen_mean"]] = din.max(), din.sum() / n_in.clamp_min(1).to(dt)
            rows[b, C["min_dist"]], rows[b, C["inside_frac"]] = d.min(), n_in.to(dt) / Nh
            rows[b, C["contact"]] = ((n_in > 0) | (d.min() <= contact_thr)).to(dt)
            counts[b, 0] = n_in.to(torch.int32)
            if want_sdf:
                out["sdf"][b], out["wind"][b] = torch.where(inside, -d, d), w
        if flags & IA_VOLUME:
            posed = can @ R.T + t
            lo = torch.maximum(hv[b].min(0)[0], posed.min(0)[0])
            hi = torch.minimum(hv[b].max(0)[0], posed.max(0)[0])
            first = torch.ceil(lo / voxel - 0.5).clamp(-1e9, 1e9).cpu().tolist()      # h (i + 1/2) in [lo, hi]
            last = torch.floor(hi / voxel - 0.5).clamp(-1e9, 1e9).cpu().tolist()
            n = [int(l) - int(f) + 1 if l >= f else 0 for f, l in zip(first, last)]
            nl = n[0] * n[1] * n[2]
            counts[b, 1] = min(nl, 2 ** 31 - 1)
            if nl > max_voxels:
                counts[b, 3] = 1
                continue
            n_both = 0
            if nl:
                ax = [voxel * (torch.arange(int(f), int(f) + k, dtype=dt, device=dev) + 0.5) for f, k in zip(first, n)]
                p = torch.stack(torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij"), -1).reshape(-1, 3).flip(-1)      # x fastest, as the kernel's index
                w_obj = orient[r] * _triangle_scan((p - t) @ R, tri, False)[0]
                in_obj = w_obj > 0.5
                w_hand = torch.full_like(w_obj, float("nan"))
                if bool(in_obj.any()):
                    w_hand[in_obj] = hand_orient * _triangle_scan(p[in_obj], hv[b][hf], False)[0]
                    n_both = int((w_hand[in_obj] > 0.5).sum())
                if want_lattice:
                    out["lattice"][b] = (p, w_obj, w_hand)
            counts[b, 2] = n_both
            rows[b, C["volume"]] = n_both * float(voxel) ** 3
    return out


def interaction_sym_values_torch(hand_verts, hand_faces, hand_orient, obj_verts, vert_off, obj_row, rot, tsl, no_max, contact_thr=0.005, want_sdf=False):
    """The definitions of ab_interaction_sym (include/artiboost_hip.h) as torch ops in hand_verts' dtype: the route of CPU tensors and, in
    float64, the reference of the tests.  Same arguments and the same dict as kernels.interaction_sym: rows [B,8] (columns
    kernels.IAS_ROW, the others NaN), counts int32 [B,2] and, with want_sdf, sdf_obj and wind_obj [B,no_max], NaN past the sample's object.
    Like the kernel it takes the hand into the object's canonical frame, triangles ((hv[b] - t) @ R)[hand_faces], and scans them for the
    canonical object vertices, one [No_r, Fh] block per sample."""
    from .kernels import IAS_ROW as C
    hv = hand_verts.detach()
    dt, dev = hv.dtype, hv.device
    B, Nh, no_max = hv.shape[0], hv.shape[1], int(no_max)
    n_obj = int(vert_off.numel()) - 1
    nan = float("nan")
    rows = torch.full((B, 8), nan, dtype=dt, device=dev)
    counts = torch.zeros((B, 2), dtype=torch.int32, device=dev)
    out = {"rows": rows, "counts": counts}
    if want_sdf:
        out["sdf_obj"], out["wind_obj"] = torch.full((B, no_max), nan, dtype=dt, device=dev), torch.full((B, no_max), nan, dtype=dt, device=dev)
    vo = [int(x) for x in vert_off.cpu()]
    orow = [min(max(int(r), 0), n_obj - 1) for r in obj_row.cpu()]
    hf = hand_faces.to(dev).long().reshape(-1, 3).clamp(0, Nh - 1)
    R_all, t_all = rot.detach().to(device=dev, dtype=dt).reshape(B, 3, 3), tsl.detach().to(device=dev, dtype=dt).reshape(B, 3)
    for b in range(B):
        r = orow[b]
        n = min(max(vo[r + 1] - vo[r], 1), no_max)
        can = obj_verts[vo[r]:vo[r] + n].to(device=dev, dtype=dt)
        tri = ((hv[b] - t_all[b]) @ R_all[b])[hf]
        w, d2 = _triangle_scan(can, tri, True)
        w, d = hand_orient * w, d2.sqrt()
        inside = w > 0.5
        n_in = inside.sum()
        din = torch.where(inside, d, torch.zeros_like(d))
        rows[b, C["obj_pen_max"]], rows[b, C["obj_pen_mean"]] = din.max(), din.sum() / n_in.clamp_min(1).to(dt)
        rows[b, C["obj_min_dist"]], rows[b, C["obj_inside_frac"]] = d.min(), n_in.to(dt) / n
        rows[b, C["obj_contact"]] = ((n_in > 0) | (d.min() <= contact_thr)).to(dt)
        counts[b, 0], counts[b, 1] = n_in.to(torch.int32), n
        if want_sdf:
            out["sdf_obj"][b, :n], out["wind_obj"][b, :n] = torch.where(inside, -d, d), w
    return out


class ObjectMeshTable:
    """The object meshes of the interaction measures as one packed table (the layout of assets.SceneAssets: verts [*,3] fp32, faces int32
    [*,3] with indices local to the object, vert_off / face_off int32 [n_obj + 1]), each mesh's orientation (the sign of its signed volume,
    float64 on the host) and the map from a batch's `obj_idx` (YCB class id) to a table row.  Faces with a repeated index are dropped here.
    Uploaded once per device (`on`).  The hand's faces and orientation travel with it (`set_hand`)."""

    def __init__(self, meshes, obj_ids, hand_model=None):
        """meshes: [(verts [V,3], faces [F,3])] in the canonical frame the poses act on (that of `corners_can`); obj_ids: their class ids."""
        vs, fs, vo, fo, orient = [], [], [0], [0], []
        for v, f in meshes:
            v, f = np.asarray(v, np.float32).reshape(-1, 3), drop_repeated_faces(f)
            if len(f) < 1 or f.min() < 0 or f.max() >= len(v):
                raise ValueError("ObjectMeshTable: every object needs at least one face, with indices inside its vertex list")
            vs.append(v); fs.append(f); vo.append(vo[-1] + len(v)); fo.append(fo[-1] + len(f)); orient.append(mesh_orientation(v, f))
        self.verts, self.faces = np.concatenate(vs), np.concatenate(fs)
        self.vert_off, self.face_off = np.asarray(vo, np.int32), np.asarray(fo, np.int32)
        self.orient = np.asarray(orient, np.float32)
        self.no_max = max(len(v) for v in vs)      # the largest vertex count of the objects (the No_max of ab_interaction_sym): a host integer
        # the closed axis-aligned box of each object's canonical vertices, lo xyz | hi xyz: minima and maxima of fp32 values, so exact in fp32
        self.box = np.stack([np.concatenate([v.min(0), v.max(0)]) for v in vs]).astype(np.float32)
        self.obj_ids = [int(i) for i in obj_ids]
        self.row_of = {i: r for r, i in enumerate(self.obj_ids)}
        lut = np.full(max(self.obj_ids + [0]) + 1, -1, np.int64)      # an id the table lacks maps to -1 (the kernel clamps it to row 0)
        lut[self.obj_ids] = np.arange(len(self.obj_ids))
        self._lut = lut
        self.hand_faces, self.hand_orient = None, 1.0
        self._dev = {}
        if hand_model is not None:
            self.set_hand(hand_model)

    @property
    def n_obj(self):
        return len(self.obj_ids)

    def set_hand(self, hand_model):
        """Hand faces from draw.hand_model_faces, the orientation from the rest-pose template."""
        from .draw import hand_model_faces
        self.hand_faces = drop_repeated_faces(hand_model_faces(hand_model))
        self.hand_orient = mesh_orientation(hand_model["v_template"], self.hand_faces)
        self._dev = {}
        return self

    @classmethod
    def from_assets(cls, assets, hand_model=None):
        """From a SceneAssets: obj_verts / obj_faces / obj_vert_off / obj_face_off / obj_idx, and its hand model."""
        vo, fo = assets.obj_vert_off, assets.obj_face_off
        meshes = [(assets.obj_verts[vo[k]:vo[k + 1]], assets.obj_faces[fo[k]:fo[k + 1]]) for k in range(len(vo) - 1)]
        return cls(meshes, list(assets.obj_idx), hand_model if hand_model is not None else assets.hand)

    @classmethod
    def from_dataset(cls, ds, hand_model=None):
        """From a dataset reader with `_verts_can` / `get_obj_faces` (datasets.HO3D): the objects its frames hold, by name, each in the
        canonical frame of `corners_can`."""
        first = {}
        for idx, i in enumerate(ds.sample_idxs):
            first.setdefault(ds.ann["obj_name"][i], idx)
        names = sorted(first)
        return cls([(ds._verts_can(o), ds.get_obj_faces(first[o])) for o in names], [ds.name2id[o] for o in names], hand_model)

    def on(self, device):
        """The table's tensors on `device`, uploaded once."""
        key = str(device)
        if key not in self._dev:
            if self.hand_faces is None:
                raise RuntimeError("ObjectMeshTable: no hand faces (set_hand)")
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)      # noqa: E731
            self._dev[key] = dict(obj_verts=t(self.verts), obj_faces=t(self.faces), vert_off=t(self.vert_off), face_off=t(self.face_off),
                                  obj_orient=t(self.orient), obj_box=t(self.box), hand_faces=t(self.hand_faces), lut=t(self._lut))
        return self._dev[key]

    def rows(self, obj_idx):
        """int64 [B] table rows of a batch's class ids, on their device, without a host read."""
        lut = self.on(obj_idx.device)["lut"]
        i = obj_idx.reshape(-1).long()
        return torch.where((i >= 0) & (i < lut.numel()), lut[i.clamp(0, lut.numel() - 1)], torch.full_like(i, -1))


IA_MEASURES = ("pen_depth_mm", "pen_mean_mm", "min_dist_mm", "inside_frac", "contact_ratio", "inter_vol_cm3", "capped")
IA_SYM_MEASURES = ("obj_pen_depth_mm", "obj_pen_mean_mm", "obj_min_dist_mm", "obj_inside_frac", "sym_pen_depth_mm", "sym_contact_ratio")      # with SYMMETRIC


@METRIC.register_module
class InteractionMetric(Metric):
    """Hand-object interaction of a prediction: means over samples of the maximum penetration depth of the hand vertices into the object
    (`pen_depth_mm`), their mean depth (`pen_mean_mm`), the smallest hand-object distance (`min_dist_mm`), the fraction of hand vertices
    inside (`inside_frac`), the fraction of samples in contact (`contact_ratio`: a vertex inside or within CONTACT_MM) and, with VOLUME, the
    intersection volume of the two meshes at VOXEL_MM voxels (`inter_vol_cm3`, over the samples whose lattice stayed within MAX_VOXELS;
    `capped` counts the others).  The hand is preds[HAND_KEY] with the hand model's faces, the object its canonical mesh under
    preds[ROT_KEY] / preds[TSL_KEY] (the rule of corners_3d_abs and MSSD), chosen by targs[obj_idx].  REPORT_GT adds the same measures of
    the annotation with a `gt_` prefix (targs: hand_verts_3d + root_joint, obj_transf).  OBJ_MESHES {SOURCE: assets, DATASET: HO3D} builds
    the stand-in table as synth.py builds its assets; `set_obj_meshes(table)` is for callers that hold the real meshes.  HIP tensors: one
    ab_interaction call per batch and group (through the evaluator's memo), nothing read back in feed_device; CPU tensors:
    interaction_values_torch in their dtype.  A batch that lacks a key is skipped and logged once.
    SYMMETRIC (default false) adds the reverse direction, the object's vertices against the hand mesh: means over
    samples of their maximum and mean depth inside the hand (`obj_pen_depth_mm`, `obj_pen_mean_mm`), their smallest distance to it
    (`obj_min_dist_mm`), the fraction of them inside (`obj_inside_frac`), the larger of the two directions' maximum depths
    (`sym_pen_depth_mm`, what the hand-object literature reports) and the fraction of samples in contact in either direction
    (`sym_contact_ratio`).  One ab_interaction_sym call per batch and group under a memo key of its own (CPU tensors:
    interaction_sym_values_torch); the one-sided call keeps its key, so a plain and a symmetric metric of one evaluator share it."""

    def __init__(self, **cfg):
        self.hand_key = cfg.get("HAND_KEY", "hand_verts_3d_abs")
        self.rot_key, self.tsl_key = cfg.get("ROT_KEY", "box_rot_rotmat"), cfg.get("TSL_KEY", "boxroot_3d_abs")
        self.contact_thr, self.voxel = float(cfg.get("CONTACT_MM", 5.0)) / 1000.0, float(cfg.get("VOXEL_MM", 5.0)) / 1000.0
        self.max_voxels, self.volume, self.report_gt = int(cfg.get("MAX_VOXELS", 262144)), bool(cfg.get("VOLUME", True)), bool(cfg.get("REPORT_GT", False))
        self.symmetric = bool(cfg.get("SYMMETRIC", False))
        if self.voxel <= 0 or self.contact_thr < 0 or not 1 <= self.max_voxels <= 1 << 24:
            raise ValueError("InteractionMetric: VOXEL_MM > 0, CONTACT_MM >= 0 and 1 <= MAX_VOXELS <= 2^24")
        self.table = None
        src = cfg.get("OBJ_MESHES")
        if src:
            if str(src.get("SOURCE", "assets")) != "assets":
                raise ValueError(f"InteractionMetric: OBJ_MESHES.SOURCE must be 'assets' (or call set_obj_meshes), got {src.get('SOURCE')!r}")
            from .assets import SceneAssets
            self.table = ObjectMeshTable.from_assets(SceneAssets(src.get("DATASET", "HO3D"), seed=1))
        self._skipped = set()
        self.reset()

    def set_obj_meshes(self, table):
        if table.hand_faces is None:
            from .hpregnet import load_hand_model
            table.set_hand(load_hand_model("assets/mano_v1_2"))
        self.table = table
        return self

    def reset(self):
        # prefix -> float64 [9]: sums of the six row slots | samples not capped | capped | samples; with SYMMETRIC six more: sums of the four
        # obj_* slots | of max(pen_max, obj_pen_max) | of max(contact, obj_contact)
        self.sums = {}

    def _inputs(self, preds, targs, prefix):
        """(hand [B,Nh,3], rot [B,3,3], tsl [B,3], obj_idx [B]) of a group, or the name of the key the batch lacks."""
        if targs.get(Queries.OBJ_IDX) is None:
            return Queries.OBJ_IDX
        if prefix == "":
            for k in (self.hand_key, self.rot_key, self.tsl_key):
                if preds.get(k) is None:
                    return k
            hand, rot, tsl = preds[self.hand_key].detach(), preds[self.rot_key].detach(), preds[self.tsl_key].detach()
        else:
            for k in ("hand_verts_3d", Queries.ROOT_JOINT, Queries.OBJ_TRANSF):
                if targs.get(k) is None:
                    return k
            T = targs[Queries.OBJ_TRANSF]
            hand, rot, tsl = targs["hand_verts_3d"] + targs[Queries.ROOT_JOINT].to(targs["hand_verts_3d"].device).unsqueeze(1), T[:, :3, :3], T[:, :3, 3]
        B = hand.shape[0]
        return hand, rot.reshape(B, 3, 3), tsl.reshape(B, 3), targs[Queries.OBJ_IDX]

    def values(self, hand, rot, tsl, obj_idx):
        """The dict of kernels.interaction for one batch: HIP tensors through ab_interaction (fp32), CPU tensors through the torch route."""
        if self.table is None:
            raise RuntimeError("InteractionMetric: no object meshes (OBJ_MESHES in the config, or set_obj_meshes)")
        from . import kernels as K
        dev = hand.device
        tb = self.table.on(dev)
        flags = K.IA_VERTS | (K.IA_VOLUME if self.volume else 0)
        dt = torch.float32 if hand.is_cuda else hand.dtype
        f = lambda t: t.to(device=dev, dtype=dt).contiguous()      # noqa: E731
        fn = K.interaction if hand.is_cuda else interaction_values_torch
        return fn(f(hand), tb["hand_faces"], self.table.hand_orient, tb["obj_verts"], tb["obj_faces"], tb["vert_off"], tb["face_off"], tb["obj_orient"],
                  self.table.rows(obj_idx.to(dev)), f(rot), f(tsl), contact_thr=self.contact_thr, voxel=self.voxel, max_voxels=self.max_voxels,
                  flags=flags)

    def values_sym(self, hand, rot, tsl, obj_idx):
        """The dict of kernels.interaction_sym for one batch: HIP tensors through ab_interaction_sym (fp32), CPU tensors through the torch route."""
        if self.table is None:
            raise RuntimeError("InteractionMetric: no object meshes (OBJ_MESHES in the config, or set_obj_meshes)")
        from . import kernels as K
        dev = hand.device
        tb = self.table.on(dev)
        dt = torch.float32 if hand.is_cuda else hand.dtype
        f = lambda t: t.to(device=dev, dtype=dt).contiguous()      # noqa: E731
        fn = K.interaction_sym if hand.is_cuda else interaction_sym_values_torch
        return fn(f(hand), tb["hand_faces"], self.table.hand_orient, tb["obj_verts"], tb["vert_off"], self.table.rows(obj_idx.to(dev)), f(rot), f(tsl),
                  self.table.no_max, contact_thr=self.contact_thr)

    def feed_device(self, preds, targs, memo=None, **kwargs):
        names, out = [], []
        for prefix in ("", "gt_") if self.report_gt else ("",):
            got = self._inputs(preds, targs, prefix)
            if isinstance(got, str):
                if (prefix, got) not in self._skipped:
                    self._skipped.add((prefix, got))
                    import logging
                    logging.getLogger("anakin").warning(f"InteractionMetric: batch without '{got}'; its {prefix or 'prediction '}measures are skipped for such batches")
                continue
            mk = ("interaction", prefix, self.hand_key, self.rot_key, self.tsl_key, self.contact_thr, self.voxel, self.max_voxels, self.volume, id(self.table))
            val = memo.get(mk) if memo is not None else None
            if val is None:
                val = self.values(*got)
                if memo is not None:
                    memo[mk] = val
            rows, cnt = val["rows"].double(), val["counts"]
            capped = cnt[:, 3] > 0
            vol = torch.where(capped | rows[:, 5].isnan(), torch.zeros_like(rows[:, 5]), rows[:, 5])
            n = torch.full((), float(rows.shape[0]), dtype=torch.float64, device=rows.device)
            names.append(prefix)
            cols = [rows[:, 0].sum(), rows[:, 1].sum(), rows[:, 2].sum(), rows[:, 3].sum(), rows[:, 4].sum(), vol.sum(),
                    (~capped).sum().double(), capped.sum().double(), n]
            if self.symmetric:
                sk = ("interaction_sym", prefix, self.hand_key, self.rot_key, self.tsl_key, self.contact_thr, id(self.table))
                sval = memo.get(sk) if memo is not None else None
                if sval is None:
                    sval = self.values_sym(*got)
                    if memo is not None:
                        memo[sk] = sval
                srows = sval["rows"].double()
                cols += [srows[:, 0].sum(), srows[:, 1].sum(), srows[:, 2].sum(), srows[:, 3].sum(),
                         torch.maximum(rows[:, 0], srows[:, 0]).sum(), torch.maximum(rows[:, 4], srows[:, 4]).sum()]
            out.append(torch.stack(cols))
        return out, names

    def feed_host(self, arrays, extra=None, **kwargs):
        for prefix, a in zip(extra or [], arrays):
            self.sums[prefix] = self.sums.get(prefix, np.zeros(15 if self.symmetric else 9)) + np.asarray(a, np.float64)

    def feed(self, preds, targs, **kwargs):
        out, names = self.feed_device(preds, targs)
        self.feed_host([t.cpu().numpy() for t in out], extra=names)

    def get_measures(self, **kwargs):
        out = {}
        for prefix, s in self.sums.items():
            n = s[8]
            if n <= 0:
                continue
            out.update({prefix + "pen_depth_mm": 1000.0 * s[0] / n, prefix + "pen_mean_mm": 1000.0 * s[1] / n, prefix + "min_dist_mm": 1000.0 * s[2] / n,
                        prefix + "inside_frac": s[3] / n, prefix + "contact_ratio": s[4] / n})
            if self.volume:
                out[prefix + "inter_vol_cm3"] = 1.0e6 * s[5] / s[6] if s[6] > 0 else float("nan")
                out[prefix + "capped"] = int(s[7])
            if self.symmetric:
                out.update({prefix + "obj_pen_depth_mm": 1000.0 * s[9] / n, prefix + "obj_pen_mean_mm": 1000.0 * s[10] / n,
                            prefix + "obj_min_dist_mm": 1000.0 * s[11] / n, prefix + "obj_inside_frac": s[12] / n,
                            prefix + "sym_pen_depth_mm": 1000.0 * s[13] / n, prefix + "sym_contact_ratio": s[14] / n})
        return out

    def __str__(self):
        return " | ".join(f"{k}: {v:6.4f}" for k, v in self.get_measures().items())


# ============================================================================ BOP average recall
def calc_pts_diameter(pts, block=512):
    """The largest distance between two of the points (bop_toolkit's misc.calc_pts_diameter), float64 on the host, in blocks of rows."""
    p = np.asarray(pts, np.float64).reshape(-1, 3)
    best = -1.0
    for s in range(0, len(p), block):
        d = p[s:s + block, None, :] - p[None, s:, :]
        best = max(best, float((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]).max()))
    return float(np.sqrt(best))


def _vsd_snap(P, K):
    """Stage A of ab_vsd on camera points P [V,3] fp32 with K [9] fp32 -> (snapped x, snapped y as python ints, Z float64 of the fp32 value, valid)."""
    from .kernels import VSD_NEAR, VSD_RANGE
    f32 = np.float32
    X, Y, Z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):
        su = np.floor((K[0] * (X / Z) + K[2]) * f32(256.0) + f32(0.5))
        sv = np.floor((K[4] * (Y / Z) + K[5]) * f32(256.0) + f32(0.5))
        valid = (Z > f32(VSD_NEAR)) & (np.abs(su) <= f32(VSD_RANGE)) & (np.abs(sv) <= f32(VSD_RANGE))
    assert su.dtype == f32 and Z.dtype == f32
    return np.where(valid, su, 0).astype(np.int64).tolist(), np.where(valid, sv, 0).astype(np.int64).tolist(), Z.astype(np.float64).tolist(), valid.tolist()


def _vsd_pose(R, t, v):
    """((r0 x + r1 y) + r2 z) + t per row, fp32."""
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    return np.stack([((R[i, 0] * x + R[i, 1] * y) + R[i, 2] * z) + t[i] for i in range(3)], 1)


def _vsd_raster(zbufs, snapped, faces, W, H):
    """Stages B and C of ab_vsd: every face of `faces` into each [H,W] fp32 z-buffer of `zbufs` (empty = +inf), one pixel block per face."""
    sx, sy, Z, ok = snapped
    for a, b, c in np.asarray(faces).reshape(-1, 3).tolist():
        if not (ok[a] and ok[b] and ok[c]):
            continue
        area = (sx[b] - sx[a]) * (sy[c] - sy[a]) - (sy[b] - sy[a]) * (sx[c] - sx[a])
        if area == 0:
            continue
        if area < 0:
            b, c, area = c, b, -area
        xs3, ys3 = (sx[a], sx[b], sx[c]), (sy[a], sy[b], sy[c])
        x0, x1 = max((min(xs3) + 255) >> 8, 0), min(max(xs3) >> 8, W - 1)
        y0, y1 = max((min(ys3) + 255) >> 8, 0), min(max(ys3) >> 8, H - 1)
        if x0 > x1 or y0 > y1:
            continue
        px, py = np.arange(x0, x1 + 1, dtype=np.int64)[None, :] * 256, np.arange(y0, y1 + 1, dtype=np.int64)[:, None] * 256
        cov, es = True, []
        for p, q in ((b, c), (c, a), (a, b)):
            dx, dy = sx[q] - sx[p], sy[q] - sy[p]
            e = dx * (py - sy[p]) - dy * (px - sx[p])
            cov = cov & ((e > 0) | ((e == 0) & (dy > 0 or (dy == 0 and dx < 0))))
            es.append(e)
        if not cov.any():
            continue
        A = np.float64(area)
        with np.errstate(all="ignore"):
            l0, l1, l2 = es[0].astype(np.float64) / A, es[1].astype(np.float64) / A, es[2].astype(np.float64) / A
            z = np.where(cov, (1.0 / ((l0 / Z[a] + l1 / Z[b]) + l2 / Z[c])).astype(np.float32), np.float32(np.inf))
        for zb in zbufs:
            sub = zb[y0:y1 + 1, x0:x1 + 1]
            np.minimum(sub, z, out=sub)


def _vsd_stage_d(de, dg, dt, K, delta, taus, diam, normalized):
    """Stage D of ab_vsd on three fp32 depth images -> [union, complement, cost per tau] as python ints."""
    f32, f64 = np.float32, np.float64
    H, W = de.shape
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    pX, pY = (xs - f64(K[2])) / f64(K[0]), (ys - f64(K[5])) / f64(K[4])
    dist = lambda d: np.sqrt((pX * d) ** 2 + (pY * d) ** 2 + d.astype(f64) ** 2)      # noqa: E731
    Le, Lg, Lt = dist(de), dist(dg), dist(dt)
    vis = lambda L: ((L.astype(f32) - Lt.astype(f32) <= f32(delta)) | (Lt == 0)) & (L > 0)      # noqa: E731
    vg = vis(Lg)
    ve = vis(Le) | (vg & (Le > 0))
    inter, uni = vg & ve, vg | ve
    dd = np.abs(Lg[inter] - Le[inter])
    if normalized:
        dd = dd / f64(diam)
    n_uni = int(uni.sum())
    return [n_uni, n_uni - int(inter.sum())] + [int((dd >= f64(f32(t))).sum()) for t in taus]


def vsd_values_numpy(obj_verts, obj_faces, vert_off, face_off, max_obj_verts, rows, rot_est, tsl_est, rot_gt, tsl_gt, cam_intr, W, H, delta, taus, diameter,
                     normalized_by_diameter=True, depth_test=None, occ_verts=None, occ_faces=None, want_depth=False):
    """The stages of ab_vsd (include/artiboost_hip.h) in numpy -- A in fp32 in the stated order, B in integers, C and D in float64 --: the route
    of CPU tensors.  Same arguments (CPU tensors or arrays) and the same dict as kernels.vsd, as CPU tensors."""
    def n(a, dt=None):
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        return a.astype(dt) if dt is not None else a
    f32 = np.float32
    verts, faces, vo, fo = n(obj_verts, f32).reshape(-1, 3), n(obj_faces).reshape(-1, 3), n(vert_off).tolist(), n(face_off).tolist()
    rows = n(rows).reshape(-1).tolist()
    B, n_obj, T = len(rows), len(vo) - 1, len(taus)
    Re, te, Rg, tg, K = n(rot_est, f32).reshape(B, 3, 3), n(tsl_est, f32).reshape(B, 3), n(rot_gt, f32).reshape(B, 3, 3), n(tsl_gt, f32).reshape(B, 3), n(cam_intr, f32).reshape(B, 9)
    diam = n(diameter, f32).reshape(-1)
    dtest = None if depth_test is None else n(depth_test, f32).reshape(B, H, W)
    occ = None if occ_verts is None else n(occ_verts, f32).reshape(B, -1, 3)
    of = None if occ_faces is None else n(occ_faces).reshape(-1, 3)
    counts, err = np.zeros((B, 2 + T), np.int32), np.ones((B, T), f32)
    depth = np.zeros((B, 3, H, W), f32)
    for b in range(B):
        r = min(max(int(rows[b]), 0), n_obj - 1)
        nv = min(vo[r + 1] - vo[r], int(max_obj_verts))
        v = verts[vo[r]:vo[r] + nv]
        f = faces[fo[r]:fo[r + 1]]
        f = f[((f >= 0) & (f < nv)).all(1)]
        zb = np.full((3, H, W), np.inf, f32)
        _vsd_raster([zb[0]], _vsd_snap(_vsd_pose(Re[b], te[b], v), K[b]), f, W, H)
        _vsd_raster([zb[1], zb[2]] if occ is not None else [zb[1]], _vsd_snap(_vsd_pose(Rg[b], tg[b], v), K[b]), f, W, H)
        zb[~np.isfinite(zb)] = 0.0
        dm = dtest[b] if dtest is not None else np.zeros((H, W), f32)
        if occ is not None:
            zt = np.full((H, W), np.inf, f32)
            _vsd_raster([zt], _vsd_snap(occ[b], K[b]), of[((of >= 0) & (of < occ.shape[1])).all(1)], W, H)
            zt[~np.isfinite(zt)] = 0.0
            dt = np.where((zb[2] > 0) & ((zt == 0) | (zb[2] < zt)), zb[2], zt)
            dt = np.where((dm > 0) & ((dt == 0) | (dm < dt)), dm, dt)
        else:
            dt = dm
        depth[b, 0], depth[b, 1], depth[b, 2] = zb[0], zb[1], dt
        c = _vsd_stage_d(zb[0], zb[1], dt, K[b], delta, taus, diam[r], normalized_by_diameter)
        counts[b] = c
        if c[0] > 0:
            err[b] = (np.asarray(c[2:], np.float64) + c[1]) / np.float64(c[0])
    out = {"counts": torch.from_numpy(counts), "err": torch.from_numpy(err)}
    if want_depth:
        out["depth"] = torch.from_numpy(depth)
    return out


def mspd_values_torch(can, obj_transf, obj_idx, sym_R, sym_t, sym_count, cam_intr, pred_R=None, pred_t=None, pred_pts=None):
    """The definition of ab_mspd as torch ops in `can`'s dtype (the route of CPU tensors; in float64 the tests' reference): per sample the
    minimum over the object's TRUE symmetry set of the maximum projection distance in pixels; +inf when a point has Z <= 0 in either pose."""
    dt, dev = can.dtype, can.device
    B, n_obj = can.shape[0], sym_R.shape[0]
    t = lambda a: a.detach().to(device=dev, dtype=dt)      # noqa: E731
    T, K = t(obj_transf).reshape(B, 4, 4), t(cam_intr).reshape(B, 3, 3)
    SR, St = t(sym_R).reshape(n_obj, -1, 3, 3), t(sym_t).reshape(n_obj, -1, 3)
    cnt, oi = sym_count.cpu().tolist(), (obj_idx.cpu() - 1).clamp(0, n_obj - 1).tolist()

    def proj(P, k):
        return torch.stack([k[0, 0] * P[..., 0] / P[..., 2] + k[0, 2], k[1, 1] * P[..., 1] / P[..., 2] + k[1, 2]], -1)
    out = torch.full((B,), float("inf"), dtype=dt, device=dev)
    for b in range(B):
        c = min(max(int(cnt[oi[b]]), 0), SR.shape[1])
        if c < 1:
            continue
        pred = t(pred_pts)[b] if pred_pts is not None else can[b] @ t(pred_R).reshape(B, 3, 3)[b].T + t(pred_t).reshape(B, 3)[b]
        Rk = T[b, :3, :3] @ SR[oi[b], :c]                                                  # [c,3,3]
        tk = St[oi[b], :c] @ T[b, :3, :3].T + T[b, :3, 3]                                  # [c,3]
        gt = torch.einsum("kij,vj->kvi", Rk, can[b]) + tk[:, None]
        if bool((pred[:, 2] <= 0).any()):
            continue
        d = torch.norm(proj(gt, K[b]) - proj(pred, K[b])[None], dim=-1)
        d = torch.where(gt[..., 2] > 0, d, torch.full_like(d, float("inf")))
        out[b] = d.max(1)[0].min()
    return out


BOP19_STEPS = np.arange(0.05, 0.51, 0.05)      # bop_toolkit's BOP19 settings: the VSD taus and every measure's ten correctness thresholds


@METRIC.register_module
class BOPRecall(Metric):
    """The BOP average recall of an object-pose prediction, AR = mean(AR_VSD, AR_MSSD, AR_MSPD) (Hodan et al., BOP Challenge 2019/2020): a
    sample is a hit of a measure at a threshold when its error is strictly below it, a measure's recall is the mean hit rate over its
    thresholds (and, for VSD, over the taus).  Defaults are the BOP19 protocol, each overridable:
      VSD    VSD_DELTA_MM 15, VSD_TAUS 0.05 .. 0.5 (normalised by the diameter: VSD_NORMALIZED), VSD_THRESHOLDS 0.05 .. 0.5
      MSSD   MSSD_THRESHOLDS 0.05 .. 0.5 x diameter
      MSPD   MSPD_THRESHOLDS 5 r .. 50 r pixels, r = IMAGE_SIZE[0] / 640
    The prediction is preds[ROT_KEY] / preds[TSL_KEY] (the rule of corners_3d_abs and MSSD), the annotation targs[obj_transf], the camera
    targs[cam_intr], images of DATA_PRESET.IMAGE_SIZE.  The symmetry table and MSSD are _MSSDBase's (MODEL_INFO / MODEL_INFO_PATH,
    MAX_SYM_DISC_STEP, MSSD_USE_CORNERS), MSPD runs over the same points; the meshes VSD renders are an ObjectMeshTable: OBJ_MESHES
    {SOURCE: assets, DATASET: HO3D} or set_obj_meshes(table).  Diameters: MODEL_INFO[i]["diameter"] (mm) when present, otherwise the largest
    distance between two vertices of the table's mesh (bop_toolkit's calc_pts_diameter), computed once on the host.
    DEPTH_TEST: `none` (no measurement: the pure est-against-gt discrepancy), `key` (targs["depth"] [B,H,W] in metres) or `hand` (the
    annotated hand targs[hand_verts_3d] + root_joint occludes, with the table's hand faces).
    HIP tensors: ab_vsd, ab_mssd and ab_mspd, once per batch through the evaluator's memo; feed_device reads nothing back: the hits are
    integer index_add_ into a device tensor [n_obj, 3, T, 10] (MSSD and MSPD use tau slot 0).  CPU tensors: vsd_values_numpy,
    the torch expression of MSSD and mspd_values_torch.  A batch that lacks a key is skipped and logged once.
    get_measures: AR, AR_VSD, AR_MSSD, AR_MSPD over all samples, `{i}.ar` per object id, and recall_vsd / recall_mssd / recall_mspd, the
    recall per threshold, as lists."""

    def __init__(self, **cfg):
        self.base = _MSSDBase(**cfg)
        self.n_obj = self.base.n_obj
        self.rot_key, self.tsl_key = cfg.get("ROT_KEY", "box_rot_rotmat"), cfg.get("TSL_KEY", "boxroot_3d_abs")
        self.image_size = [int(s) for s in cfg["DATA_PRESET"]["IMAGE_SIZE"]]
        self.delta = float(cfg.get("VSD_DELTA_MM", 15.0)) / 1000.0
        self.taus = [float(t) for t in cfg.get("VSD_TAUS", BOP19_STEPS)]
        self.normalized = bool(cfg.get("VSD_NORMALIZED", True))
        r = self.image_size[0] / 640.0
        self.thresholds = np.stack([np.asarray(cfg.get("VSD_THRESHOLDS", BOP19_STEPS), np.float64), np.asarray(cfg.get("MSSD_THRESHOLDS", BOP19_STEPS), np.float64),
                                    np.asarray(cfg.get("MSPD_THRESHOLDS", [r * k for k in range(5, 51, 5)]), np.float64)])      # [3, n_thr]
        self.depth_test = str(cfg.get("DEPTH_TEST", "none"))
        from .kernels import VSD_MAX_TAUS
        if self.depth_test not in ("none", "key", "hand") or not 1 <= len(self.taus) <= VSD_MAX_TAUS or self.delta < 0:
            raise ValueError("BOPRecall: DEPTH_TEST is one of none / key / hand, 1 to 16 VSD_TAUS, VSD_DELTA_MM >= 0")
        import json
        info = cfg.get("MODEL_INFO") or json.load(open(cfg["MODEL_INFO_PATH"], "r"))
        self._info_diam = [info[str(i)].get("diameter") for i in range(1, self.n_obj + 1)]
        self.table, self._diam, self._tens = None, None, {}
        src = cfg.get("OBJ_MESHES")
        if src:
            if str(src.get("SOURCE", "assets")) != "assets":
                raise ValueError(f"BOPRecall: OBJ_MESHES.SOURCE must be 'assets' (or call set_obj_meshes), got {src.get('SOURCE')!r}")
            from .assets import SceneAssets
            self.set_obj_meshes(ObjectMeshTable.from_assets(SceneAssets(src.get("DATASET", "HO3D"), seed=1)))
        self._skipped = set()
        self.reset()

    def set_obj_meshes(self, table):
        if table.hand_faces is None and self.depth_test == "hand":
            from .hpregnet import load_hand_model
            table.set_hand(load_hand_model("assets/mano_v1_2"))
        self.table = table
        d = np.full(self.n_obj, np.nan)                                               # metres, by 1-based object id
        for i in range(1, self.n_obj + 1):
            if self._info_diam[i - 1] is not None:
                d[i - 1] = float(self._info_diam[i - 1]) / 1000.0
            elif i in table.row_of:
                r = table.row_of[i]
                d[i - 1] = calc_pts_diameter(table.verts[table.vert_off[r]:table.vert_off[r + 1]])
        self._diam = d
        self._row_diam = np.asarray([d[i - 1] if 1 <= i <= self.n_obj else np.nan for i in table.obj_ids], np.float32)
        self.max_obj_verts = int((table.vert_off[1:] - table.vert_off[:-1]).max())
        self._tens = {}
        return self

    def reset(self):
        self._hits = self._cnt = None
        self.count = 0

    def _on(self, dev):
        """The metric's own small tensors on `dev`, uploaded once (the mesh table keeps its own cache, without the hand faces when it has none)."""
        key = str(dev)
        if key not in self._tens:
            tb, t = self.table, lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
            lut = torch.from_numpy(tb._lut).to(dev)
            self._tens[key] = dict(obj_verts=t(tb.verts), obj_faces=t(tb.faces), vert_off=t(tb.vert_off), face_off=t(tb.face_off), lut=lut,
                                   hand_faces=None if tb.hand_faces is None else t(tb.hand_faces), row_diam=t(self._row_diam), diam=t(self._diam),
                                   thr=t(self.thresholds))
        return self._tens[key]

    def _missing(self, preds, targs):
        need_t = [Queries.OBJ_IDX, Queries.OBJ_TRANSF, Queries.CAM_INTR, Queries.CORNERS_CAN if self.base.mssd_use_corners else "obj_verts_can"]
        need_p = [self.rot_key, self.tsl_key] + (["corners_3d_abs"] if self.base.mssd_use_corners else [])
        need_p += ["joints_3d_abs"] if self.base.center_idx is not None else []
        need_t += [Queries.ROOT_JOINT] if self.base.center_idx is not None else []
        need_t += {"none": [], "key": ["depth"], "hand": ["hand_verts_3d", Queries.ROOT_JOINT]}[self.depth_test]
        for k in need_p:
            if preds.get(k) is None:
                return k
        for k in need_t:
            if targs.get(k) is None:
                return k
        return None

    def values(self, preds, targs):
        """One batch -> dict: obj_idx int64 [B] (1-based), vsd_counts int32 [B,2+T], mssd [B] (metres), mspd [B] (pixels), on the predictions' device."""
        if self.table is None:
            raise RuntimeError("BOPRecall: no object meshes (OBJ_MESHES in the config, or set_obj_meshes)")
        from . import kernels as K
        rot = preds[self.rot_key].detach()
        dev, B = rot.device, rot.shape[0]
        tn = self._on(dev)
        hip = rot.is_cuda
        dt = torch.float32 if hip else rot.dtype
        f = lambda x: x.detach().to(device=dev, dtype=torch.float32).contiguous()      # noqa: E731
        obj_idx = targs[Queries.OBJ_IDX].to(dev).long().reshape(-1)
        lut = tn["lut"]
        rows = torch.where((obj_idx >= 0) & (obj_idx < lut.numel()), lut[obj_idx.clamp(0, lut.numel() - 1)], torch.full_like(obj_idx, -1))
        T = targs[Queries.OBJ_TRANSF].to(dev)
        W, H = self.image_size
        kw = dict(depth_test=None, occ_verts=None, occ_faces=None)
        if self.depth_test == "key":
            kw["depth_test"] = f(targs["depth"]).reshape(B, H, W)
        elif self.depth_test == "hand":
            kw["occ_verts"] = f(targs["hand_verts_3d"].to(dev) + targs[Queries.ROOT_JOINT].to(dev).unsqueeze(1))
            kw["occ_faces"] = tn["hand_faces"]
        fn = K.vsd if hip else vsd_values_numpy
        v = fn(tn["obj_verts"], tn["obj_faces"], tn["vert_off"], tn["face_off"], self.max_obj_verts, rows.contiguous(), f(rot).reshape(B, 3, 3),
               f(preds[self.tsl_key]).reshape(B, 3), f(T[:, :3, :3]), f(T[:, :3, 3]), f(targs[Queries.CAM_INTR]).reshape(B, 3, 3), W, H, self.delta, self.taus,
               tn["row_diam"], normalized_by_diameter=self.normalized, **kw)
        _, mssd = self.base.values(preds, targs)
        can = targs[Queries.CORNERS_CAN if self.base.mssd_use_corners else "obj_verts_can"].to(dev)
        if self.base.mssd_use_corners:
            mode = dict(pred_pts=preds["corners_3d_abs"].detach())
        else:
            mode = dict(pred_R=rot.reshape(B, 3, 3), pred_t=preds[self.tsl_key].detach().reshape(B, 3))
        g = (lambda x: f(x)) if hip else (lambda x: x.detach().to(dt))
        args = (g(can), g(T), obj_idx.contiguous(), self.base.R, self.base.t, self.base.sym_count, g(targs[Queries.CAM_INTR].to(dev)))
        mspd = (K.mspd if hip else mspd_values_torch)(*args, **{k: g(x) for k, x in mode.items()})
        return dict(obj_idx=obj_idx, vsd_counts=v["counts"].to(dev), mssd=mssd, mspd=mspd)

    def hits(self, val, dev):
        """int64 [B, 3, T, n_thr] of one batch's values: strict `<`, in float64.  The VSD error is formed from the integer counts in float64, as
        bop_toolkit forms it, so a sample exactly on a threshold falls where it falls there."""
        tn = self._on(dev)
        thr = tn["thr"]                                                                  # [3, n_thr] float64
        c = val["vsd_counts"].to(torch.float64)
        uni = c[:, 0:1]
        e = torch.where(uni > 0, (c[:, 2:] + c[:, 1:2]) / uni.clamp_min(1.0), torch.ones_like(c[:, 2:]))      # [B,T]
        B, T, n = e.shape[0], e.shape[1], thr.shape[1]
        out = torch.zeros((B, 3, T, n), dtype=torch.int64, device=dev)
        out[:, 0] = (e[:, :, None] < thr[0][None, None, :]).to(torch.int64)
        oi = (val["obj_idx"] - 1).clamp(0, self.n_obj - 1)
        diam = tn["diam"][oi]                                                            # NaN for an object without a diameter: never a hit
        out[:, 1, 0] = (val["mssd"].to(torch.float64)[:, None] < thr[1][None, :] * diam[:, None]).to(torch.int64)
        out[:, 2, 0] = (val["mspd"].to(torch.float64)[:, None] < thr[2][None, :]).to(torch.int64)
        return out, oi

    def feed_device(self, preds, targs, memo=None, **kwargs):
        miss = self._missing(preds, targs)
        if miss is not None:
            if miss not in self._skipped:
                self._skipped.add(miss)
                import logging
                logging.getLogger("anakin").warning(f"BOPRecall: batch without '{miss}'; such batches are skipped")
            return []
        mk = ("bop", id(self), id(self.table))
        val = memo.get(mk) if memo is not None else None
        if val is None:
            val = self.values(preds, targs)
            if memo is not None:
                memo[mk] = val
        dev = val["mssd"].device
        h, oi = self.hits(val, dev)
        if self._hits is None or self._hits.device != dev:
            self._hits = torch.zeros((self.n_obj,) + tuple(h.shape[1:]), dtype=torch.int64, device=dev)
            self._cnt = torch.zeros(self.n_obj, dtype=torch.int64, device=dev)
        self._hits.index_add_(0, oi, h)
        self._cnt.index_add_(0, oi, torch.ones_like(oi))
        return [torch.full((1,), h.shape[0], dtype=torch.int64, device=dev)]

    def feed_host(self, arrays, **kwargs):
        for a in arrays:
            self.count += int(a[0])

    def feed(self, preds, targs, **kwargs):
        self.feed_host([t.cpu().numpy() for t in self.feed_device(preds, targs)])

    def get_measures(self, **kwargs):
        if self._hits is None:
            return {}
        h, c = self._hits.cpu().numpy().astype(np.float64), self._cnt.cpu().numpy().astype(np.float64)
        n, T = c.sum(), h.shape[2]
        if n <= 0:
            return {}
        rec = [h[:, 0].sum(0).sum(0) / (n * T), h[:, 1, 0].sum(0) / n, h[:, 2, 0].sum(0) / n]      # per threshold
        out = {"AR_VSD": float(rec[0].mean()), "AR_MSSD": float(rec[1].mean()), "AR_MSPD": float(rec[2].mean())}
        out["AR"] = (out["AR_VSD"] + out["AR_MSSD"] + out["AR_MSPD"]) / 3.0
        for i in np.nonzero(c)[0]:
            out[f"{i + 1}.ar"] = float((h[i, 0].mean() + h[i, 1, 0].mean() + h[i, 2, 0].mean()) / (3.0 * c[i]))
        out.update(recall_vsd=rec[0].tolist(), recall_mssd=rec[1].tolist(), recall_mspd=rec[2].tolist())
        return out

    def __str__(self):
        m = self.get_measures() if self.count else {}
        return " | ".join(f"{k}: {m[k]:6.4f}" for k in ("AR", "AR_VSD", "AR_MSSD", "AR_MSPD") if k in m)
