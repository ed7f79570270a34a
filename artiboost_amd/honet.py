"""HoNet (anakin/models/honetMANO.py:19-286): the hand-mesh + object-vertices model of the registry -- ResNet-18 features -> ManoBranch
(hand) + two TransHeads: `mano_transhead` (scale, 2-D translation of the hand) and `obj_transhead` (scale, 2-D translation, axis-angle
of the object).  Unlike HOPRegNet it places the hand from the PREDICTED scale / translation (`recover_3d_proj`), reads the canonical
object vertices (Queries.OBJ_VERTS_CAN) and returns `obj_verts_3d_abs`, which ObjLoss consumes.

This is the plain torch module (CPU, or any torch device); with cfg["DEVICE"] naming a HIP device `HoNet(**cfg)` builds
regnet.HoNetHIP, the same model on the HIP kernels.  `manotorch.utils.rodrigues.rodrigues` (third party, un-pinned, absent) is
replaced by hpregnet._rodrigues: parity with the reference is unpinned at exactly that call."""
import os

import torch
import torch.nn as nn

from .hpregnet import HOPRegNet, _rodrigues, batch_persp_proj2d
from .registry import MODEL, Queries, build_backbone, build_head, enable_lower_param


@MODEL.register_module
class HoNet(nn.Module):
    class TransHead(nn.Module):
        def __init__(self, inp_dim, out_dim):
            super().__init__()
            if out_dim not in (3, 6):
                raise ValueError(f"Unrecognized TransHead out dim: {out_dim}")
            self.final_layer = nn.Linear(inp_dim // 2, out_dim)
            self.decoder = nn.Sequential(nn.Linear(inp_dim, inp_dim // 2), nn.ReLU())

        def forward(self, inp):
            return self.final_layer(self.decoder(inp))

    def __new__(cls, *args, **cfg):
        """cfg["DEVICE"] naming a HIP device builds the model on the HIP kernels (regnet.HoNetHIP), as HOPRegNet.__new__ does."""
        dev = cfg.get("DEVICE", cfg.get("device"))
        if cls is HoNet and dev is not None and torch.device(dev).type in ("cuda", "hip"):
            from .regnet import HoNetHIP
            return HoNetHIP(*args, **cfg)
        return super().__new__(cls)

    @enable_lower_param
    def __init__(self, **cfg):
        super().__init__()
        self.inp_res = cfg["DATA_PRESET"]["IMAGE_SIZE"]
        self.feature_dim = cfg["HEAD"]["INPUT_DIM"]
        self.center_idx = cfg["DATA_PRESET"]["CENTER_IDX"]
        if cfg.get("MANO_FHB_ADAPTOR", False):
            raise NotImplementedError("MANO_FHB_ADAPTOR (FPHAB skeleton adaptor, honetMANO.py:44-51)")
        self.base_net = build_backbone(cfg["BACKBONE"])
        self.mano_branch = build_head(cfg["HEAD"], default_args=cfg["DATA_PRESET"])
        self.obj_trans_factor = cfg["OBJ_TRANS_FACTOR"]
        self.obj_scale_factor = cfg["OBJ_SCALE_FACTOR"]
        self.mano_transhead = HoNet.TransHead(self.feature_dim, 3)
        self.obj_transhead = HoNet.TransHead(self.feature_dim, 6)
        self.proj2d_func = batch_persp_proj2d
        self.adaptor = None
        pretrained = cfg.get("PRETRAINED", "")
        if pretrained:
            if not os.path.isfile(pretrained):
                raise FileNotFoundError(f"=> No {type(self).__name__} checkpoints file found in {pretrained}")
            ck = torch.load(pretrained, map_location="cpu")
            self.load_state_dict(ck["state_dict"] if isinstance(ck, dict) and "state_dict" in ck else ck, strict=True)

    @staticmethod
    def remap_hasson_state_dict(sd):
        """honetMANO.py:78-111: checkpoints of Hasson et al. (CVPR 2020) name the left MANO layer (dropped), `mano_layer_right`
        (-> `mano_layer`), `scaletrans_branch_obj` (-> `obj_transhead`) and `scaletrans_branch.` (-> `mano_transhead.`)."""
        out = {}
        for k, v in sd.items():
            if "mano_layer_left" in k:
                continue
            if "mano_layer_right" in k:
                k = k.replace("mano_layer_right", "mano_layer")
            elif "scaletrans_branch_obj" in k:
                k = k.replace("scaletrans_branch_obj", "obj_transhead")
            elif "scaletrans_branch." in k:
                k = k.replace("scaletrans_branch", "mano_transhead")
            out[k] = v
        return out

    @classmethod
    def clean_reference_state_dict(cls, sd):
        """Reference / Hasson checkpoint -> the keys this module owns: the remapping above, then HOPRegNet's cleaning (the `module.`
        prefix and the MANO asset buffers `mano_branch.mano_layer.*` go; the constants come from the assets)."""
        return HOPRegNet.clean_reference_state_dict(cls.remap_hasson_state_dict(sd))

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        clean = self.remap_hasson_state_dict(state_dict)
        if prefix == "":
            clean = HOPRegNet.clean_reference_state_dict(clean)
        else:
            clean = {k: v for k, v in clean.items() if not k.startswith(prefix + HOPRegNet.MANO_LAYER_PREFIX)}
        state_dict.clear()
        state_dict.update(clean)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    @staticmethod
    def recover_3d_proj(objpoints3d, camintr, est_scale, est_trans, input_res, off_z=0.4):
        """Centred points, camera intrinsics and a predicted scale / translation in pixel space -> the points in the camera frame and
        their centre (honetMANO.py:113-139)."""
        focal = camintr[:, :1, :1]
        batch_size = objpoints3d.shape[0]
        focal = focal.view(batch_size, 1)
        est_scale = est_scale.view(batch_size, 1)
        est_trans = est_trans.view(batch_size, 2)
        est_Z0 = focal * est_scale + off_z
        cam_centers = camintr[:, :2, 2]
        img_centers = (cam_centers.new(input_res) / 2).view(1, 2).repeat(batch_size, 1)
        est_XY0 = (est_trans + img_centers - cam_centers) * est_Z0 / focal
        est_c3d = torch.cat([est_XY0, est_Z0], -1).unsqueeze(1)
        return est_c3d + objpoints3d, est_c3d

    def recover_mano(self, feature, samples):
        res = self.mano_branch(feature)
        scaletrans = self.mano_transhead(feature)
        trans, scale = scaletrans[:, 1:], scaletrans[:, :1]
        final_trans = trans.unsqueeze(1) * self.obj_trans_factor
        final_scale = scale.view(scale.shape[0], 1, 1) * self.obj_scale_factor
        height, width = tuple(samples[Queries.IMAGE].shape[2:])
        cam_intr = samples[Queries.CAM_INTR].to(feature.device)
        joints_3d_abs, root_joint = HoNet.recover_3d_proj(res["joints_3d"], cam_intr, final_scale, final_trans, input_res=(width, height))
        hand_verts_3d_abs = res["hand_verts_3d"] + root_joint
        res.update(joints_2d=self.proj2d_func(joints_3d_abs, cam_intr), root_joint=root_joint, joints_3d_abs=joints_3d_abs,
                   hand_verts_3d_abs=hand_verts_3d_abs, hand_verts_2d=self.proj2d_func(hand_verts_3d_abs, cam_intr),
                   hand_pred_trans=trans, hand_pred_scale=scale, hand_trans=final_trans, hand_scale=final_scale)
        return res

    def recover_object(self, feature, samples):
        st = self.obj_transhead(feature)
        B, dev = st.shape[0], feature.device
        scale, trans, rotaxisang = st[:, :1], st[:, 1:3], st[:, 3:]
        rotmat = _rodrigues(rotaxisang).view(B, 3, 3)
        can = samples[Queries.OBJ_VERTS_CAN].to(dev)
        obj_verts_ = rotmat.bmm(can.float().transpose(1, 2)).transpose(1, 2)
        final_trans = trans.unsqueeze(1) * self.obj_trans_factor
        final_scale = scale.view(B, 1, 1) * self.obj_scale_factor
        height, width = tuple(samples[Queries.IMAGE].shape[2:])
        cam_intr = samples[Queries.CAM_INTR].to(dev)
        obj_verts_3d_abs, obj_center = HoNet.recover_3d_proj(obj_verts_, cam_intr, final_scale, final_trans, input_res=(width, height))
        if Queries.CORNERS_3D in samples:
            corners_ = rotmat.bmm(samples[Queries.CORNERS_CAN].to(dev).float().transpose(1, 2)).transpose(1, 2)
            corners_3d_abs = corners_ + obj_center
            corners_2d = self.proj2d_func(corners_3d_abs, cam_intr)
        else:
            corners_3d_abs = corners_2d = None
        return {"obj_center": obj_center, "obj_verts_3d_abs": obj_verts_3d_abs, "corners_3d_abs": corners_3d_abs, "obj_pred_scale": scale,
                "obj_pred_trans": trans, "obj_rot": rotaxisang, "obj_scale": final_scale, "obj_trans": final_trans, "corners_2d": corners_2d,
                "obj_verts_2d": self.proj2d_func(obj_verts_3d_abs, cam_intr), "box_rot_rotmat": rotmat, "boxroot_3d_abs": obj_center}

    def forward(self, samples):
        dev = next(self.parameters()).device
        feat = self.base_net(image=samples["image"].to(dev))["res_layer4_mean"]
        mano, obj = self.recover_mano(feat, samples), self.recover_object(feat, samples)
        # root-relative object; without CORNERS_3D the corner entries are None (the reference's subtraction has no operand then)
        obj["corners_3d"] = None if obj["corners_3d_abs"] is None else obj["corners_3d_abs"] - mano["root_joint"]
        obj["obj_verts_3d"] = obj["obj_verts_3d_abs"] - mano["root_joint"]
        return {**mano, **obj}
