"""Evaluation / submission pass: anakin/submit/hodata_submit_epoch_pass.py:21-156 and
submit_epoch_pass.py -- eval-mode forward over a loader, metrics, and the HO3D-v2 CodaLab prediction file.

Without mesh fitting the vertex half of the file is zeros, as in the reference.  With FIT_MESH (`--postprocess_fit_mesh`) the
vertices come from `fitting.FittingUnit` (IKNet + 20 Adam steps of a MANO fit per hand, one `ab_mano_fit` launch per batch on a
HIP device) and are written as they are, in the predicted camera frame -- unlike the joints, they get no OpenGL flip (the
reference's own convention, hodata_submit_epoch_pass.py:148-149).  FIT_MESH_USE_FITTED_JOINTS writes the fitted joints instead of
the predicted ones, with the joint reorder undone and y and z negated (:129-140).  With FIT_MESH and DRAW (`--postprocess_draw`) every
frame also gets a four-panel PNG under `draw_path` (:109-123, :158-218): `draw.MeshDrawer` rasterises the two mesh panels of the whole
batch on the device (`ab_draw_meshes`) and draws the two skeleton panels on the host.  Those pixels are this build's own (DESIGN.md
section 18), not OpenDR's / mayavi's / matplotlib's."""
import json
import os
import warnings
import zipfile

import numpy as np
import torch


class HOSubmitEpochPass:
    """SubmitEpochPass.reg("hodata").  cfg: {"DUMP": bool, "TRUE_ROOT": bool (arg.true_root), "FIT_MESH": bool,
    "FIT_MESH_USE_FITTED_JOINTS": bool, "FIT_MESH_IK": "iknet" | "iksolver", "DRAW": bool (arg.postprocess_draw),
    "FITTING_UNIT": a FittingUnit-like callable to use instead of building one, "DRAWER": a MeshDrawer-like object (`draw_batch`) to use
    instead of building one, "DRAW_PATH": the directory of the drawings (arg.postprocess_draw_path; default: the call's draw_path)}."""

    def __init__(self, cfg=None):
        cfg = cfg or {}
        self.dump = cfg.get("DUMP", True)
        self.true_root = cfg.get("TRUE_ROOT", False)
        self.fit_mesh = bool(cfg.get("FIT_MESH", False))
        self.fit_mesh_use_fitted_joints = bool(cfg.get("FIT_MESH_USE_FITTED_JOINTS", False))
        # "iksolver" is accepted and ignored, as in the reference: its FittingUnit always initialises with IKNet
        self.fit_mesh_ik = cfg.get("FIT_MESH_IK", "iknet")
        self.fitting_unit = None
        # DRAW without FIT_MESH is a silent no-op, as in the reference (:109).  The drawer is built at the first batch: nothing here touches the device.
        self.draw = self.fit_mesh and bool(cfg.get("DRAW", False))
        self.drawer, self.draw_path, self.sample_counter = cfg.get("DRAWER"), cfg.get("DRAW_PATH"), 0
        if self.fit_mesh:
            if self.draw:
                msg = ("--postprocess_draw: the drawings come from this build's own rasteriser (ab_draw_meshes), not from OpenDR / mayavi / "
                       "matplotlib; they are not pixel-comparable with the reference's")
                if self.drawer is None and not torch.cuda.is_available():
                    self.draw = False
                    msg += "; no HIP device is visible, so they are skipped"
                warnings.warn(msg)
            self.fitting_unit = cfg.get("FITTING_UNIT")
            if self.fitting_unit is None:
                from .fitting import FittingUnit
                self.fitting_unit = FittingUnit()

    @staticmethod
    def get_order_idxs():
        reorder_idxs = [0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20]
        return reorder_idxs, np.argsort(reorder_idxs)

    @staticmethod
    def dump_json(pred_out_path, xyz_pred_list, verts_pred_list, codalab=True):
        """hodata_submit_epoch_pass.py:34-56: [joints, verts] rounded to 5 decimals; zipped for CodaLab (zipfile instead
        of the `zip` binary, same single flat entry as `zip -j`)."""
        def roundall(rows):
            return [[round(val, 5) for val in row] for row in rows]
        xyz = [roundall(x.tolist()) for x in xyz_pred_list]
        verts = [roundall(x.tolist()) for x in verts_pred_list]
        with open(pred_out_path, "w") as fo:
            json.dump([xyz, verts], fo)
        if codalab:
            with zipfile.ZipFile(pred_out_path.replace(".json", ".zip"), "w", zipfile.ZIP_DEFLATED) as z:
                z.write(pred_out_path, os.path.basename(pred_out_path))

    def _hand_faces(self):
        """The reference's FittingUnit.face: the closed-wrist faces of hand_face_path when that file exists, else the model's 1538."""
        path = getattr(self.fitting_unit, "hand_face_path", None) or "assets/postprocess/hand_close.npy"
        if os.path.isfile(path):
            return np.load(path)
        from .hpregnet import load_hand_model
        from .draw import hand_model_faces
        return hand_model_faces(load_hand_model(getattr(self.fitting_unit, "mano_root", "assets/mano_v1_2")))

    def _draw_batch(self, batch, predicts, fitted_verts, dataset, draw_path):
        if self.drawer is None:
            from .draw import MeshDrawer
            self.drawer = MeshDrawer(self._hand_faces(), image_size=tuple(batch["image"].shape[-2:][::-1]))
        n = batch["image"].shape[0]
        tsl = predicts.get("boxroot_3d_abs")
        self.sample_counter = self.drawer.draw_batch(
            batch["image"], batch["cam_intr"], batch.get("sample_idx", torch.arange(self.sample_counter, self.sample_counter + n)),
            predicts["joints_3d_abs"].detach(), fitted_verts, predicts.get("box_rot_rotmat"), None if tsl is None else tsl.reshape(n, 3),
            predicts.get("corners_3d_abs"), dataset, self.draw_path or draw_path, self.sample_counter)

    def __call__(self, epoch_idx, data_loader, arch_model, criterion=None, evaluator=None, rank=0, dump_path=None, draw_path=None):
        arch_model.eval()
        if evaluator:
            evaluator.reset_all()
        res_joints, res_verts = [], []
        _, unorder = self.get_order_idxs()
        with torch.no_grad():
            for batch in data_loader:
                predicts = {}
                for preds in arch_model(batch).values():
                    predicts.update(preds)
                if criterion:
                    _, losses = criterion.compute_losses(predicts, batch)
                else:
                    losses = {}
                if self.true_root:
                    predicts["joints_3d_abs"][:, 0] = batch["root_joint"].to(predicts["joints_3d_abs"].device)
                if evaluator:
                    evaluator.feed_all(predicts, batch, losses)
                if self.fit_mesh:
                    fit = getattr(self.fitting_unit, "fit", None)
                    if self.draw and fit is not None and (self.draw_path or draw_path):
                        # one fit, its device tensors kept for the drawer; the host lists as FittingUnit.__call__ returns them
                        dv, dj = fit(predicts["joints_3d_abs"].detach())
                        fitted_verts, fitted_joints = list(dv.cpu().numpy()), list(dj.cpu().numpy())
                    else:
                        dv = None
                        fitted_verts, fitted_joints = self.fitting_unit(batch, predicts["joints_3d_abs"].detach())
                    if self.draw and (self.draw_path or draw_path):
                        self._draw_batch(batch, predicts, dv if dv is not None else fitted_verts, getattr(data_loader, "dataset", None),
                                         draw_path)
                if self.fit_mesh and self.fit_mesh_use_fitted_joints:
                    # hodata_submit_epoch_pass.py:129-140: reorder undone, y and z negated (no x flip, no overall sign)
                    for fj in fitted_joints:
                        item = np.array(fj[unorder, :])
                        item[:, 1] = -item[:, 1]
                        item[:, 2] = -item[:, 2]
                        res_joints.append(item)
                else:
                    # HO3D submission convention (hodata_submit_epoch_pass.py:141-145): undo the joint reorder, OpenGL axes
                    pj = predicts["joints_3d_abs"].detach().cpu()[:, unorder].clone()
                    pj[:, :, 0] = -pj[:, :, 0]
                    joints = [-val.numpy()[0] for val in pj.split(1)]
                    res_joints.extend(joints)
                if self.fit_mesh:
                    res_verts.extend(fitted_verts)
                else:
                    res_verts.extend([np.zeros((778, 3))] * len(joints))
        if self.dump and dump_path:
            self.dump_json(dump_path, res_joints, res_verts, codalab=True)
        return res_joints


class SubmitEpochPass:
    """anakin/submit/submit_epoch_pass.py: `SubmitEpochPass.build(arg.submit_dataset, cfg=None)` (train/submit_reload.py:38)."""
    _types = {"hodata": HOSubmitEpochPass}

    @classmethod
    def build(cls, type, cfg=None):
        if type not in cls._types:
            raise NotImplementedError(f"SubmitEpochPass of type {type} is not implemented")
        return cls._types[type](cfg)
