"""DiscoNet student (LiDAROnly/lidar_disco.yaml, `model.core_method: point_pillar_disconet`): host mirror of
opencood/models/point_pillar_disconet.py:19-96.  Old-style PointPillars on the `processed_lidar` key, DiscoFusion over the
agents of every scene, anchor heads -- and the fused map returned as `feature`, which PointPillarDiscoNetLoss distils against
the early-fusion teacher's (point_pillar_disconet_teacher.py).  Same constructor `args` and state_dict names as the reference
(`pillar_vfe.*`, `backbone.*`, `shrink_conv.*`, `fusion_net.pixel_weight_layer.*`, `cls_head / reg_head / dir_head.*`).
`fusion_net` is the existing DiscoFusion: inference on the device runs heal_disco_fuse, training its torch arithmetic."""
from heal_amd.opencood.models.fuse_modules.fusion_in_one import DiscoFusion
from heal_amd.opencood.models.point_pillar import _PillarDetector
from heal_amd.opencood.utils.transformation_utils import normalize_pairwise_tfm


class PointPillarDiscoNet(_PillarDetector):
    def before_heads(self, args):
        self.discrete_ratio = args["voxel_size"][0]
        self.fusion_net = DiscoFusion(self.out_channel)

    def forward(self, data_dict):
        """point_pillar_disconet.py:51-96.  The reference also unpacks `teacher_processed_lidar` and `lidar_pose` here and uses
        neither (:57-62); they are not required."""
        canvas, x = self.bev_features(data_dict)
        affine_matrix = normalize_pairwise_tfm(data_dict["pairwise_t_matrix"], canvas.shape[2], canvas.shape[3],
                                               self.voxel_size[0])
        x = self.fusion_net(x, data_dict["record_len"], affine_matrix)
        out = {"feature": x}
        out.update(self.predictions(x))
        return out
