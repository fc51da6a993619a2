"""DiscoNet teacher (`kd_flag.teacher_model: point_pillar_disconet_teacher`): host mirror of
opencood/models/point_pillar_disconet_teacher.py:14-69.  An early-fusion PointPillars: it reads
`data_dict['teacher_processed_lidar']`, the voxels of every agent's cloud projected into the ego frame and stacked, one sample
per scene (intermediate_fusion_dataset.py:391-400; heal_amd.synth.teacher_points builds the same input), and returns its map
and heads under `teacher_*` names.

`dir_preds` is returned UNPREFIXED, as in the reference (:65-66): under train_w_kd.py:144-146 (`output_dict.update(teacher_output)`)
it overwrites the student's `dir_preds`, so the direction loss of that script is computed on the frozen teacher's output and
the student's direction head receives no gradient.  Mirrored faithfully."""
from heal_amd.opencood.models.point_pillar import _PillarDetector


class PointPillarDiscoNetTeacher(_PillarDetector):
    def encode_processed_lidar(self, data_dict):
        return super().encode_processed_lidar({"processed_lidar": data_dict["teacher_processed_lidar"]})

    def forward(self, data_dict):
        x = self.bev_features(data_dict)[1]
        heads = self.predictions(x)
        out = {"teacher_feature": x, "teacher_cls_preds": heads["cls_preds"], "teacher_reg_preds": heads["reg_preds"]}
        if self.use_dir:
            out["dir_preds"] = heads["dir_preds"]
        return out
