"""DiscoNet's loss (`loss.core_method: point_pillar_disconet_loss`): host mirror of
opencood/loss/point_pillar_disconet_loss.py:11-112 -- PointPillarLoss plus kd['weight'] x the KL divergence between the channel
softmax of the student's fused map (`feature`) and the teacher's (`teacher_feature`), mean over elements.

On the device the KL term and its gradient are ONE pass of heal_kd_kl_loss over the two NCHW maps (ops.KdKlLoss) instead of the
reference's permuted copies, log_softmax, softmax, kl_div, mean and their backward; CPU tensors, other dtypes, a teacher that
carries gradient and HEAL_KD_FUSED=0 take the reference's torch composition (ops.kd_kl_torch).

`kd.decoder_kd: true` is refused: the reference's branch (:48-63) cannot run -- it calls `.permuate` and reads an undefined
`teacher_psm` -- so there is no behaviour to mirror."""
from heal_amd import ops
from heal_amd.opencood.loss.point_pillar_loss import PointPillarLoss


class PointPillarDiscoNetLoss(PointPillarLoss):
    _LOG_FIELDS = PointPillarLoss._LOG_FIELDS + (("KD Loss", "kd_loss", "Kd_loss"),)

    def __init__(self, args):
        super().__init__(args)
        self.kd = args['kd']
        if self.kd.get('decoder_kd', False):
            raise NotImplementedError("kd.decoder_kd: the reference's decoder distillation (point_pillar_disconet_loss.py:48-63) "
                                      "cannot run (`.permuate`, undefined `teacher_psm`); only the feature KL term is built")

    @staticmethod
    def kd_term(feature, teacher_feature):
        if ops.kd_kl_supported(feature, teacher_feature):
            return ops.KdKlLoss.apply(feature, teacher_feature)
        return ops.kd_kl_torch(feature, teacher_feature)

    def forward(self, output_dict, target_dict):
        total_loss = super().forward(output_dict, target_dict)
        kd_loss = self.kd_term(output_dict['feature'], output_dict['teacher_feature']) * self.kd['weight']
        total_loss = total_loss + kd_loss
        self.loss_dict.update({'total_loss': total_loss.item(), 'kd_loss': kd_loss.item()})
        return total_loss
