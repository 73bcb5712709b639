"""WSGANBiGANModel -- the reference's BiGAN-style model (models/wsgan_bigan_model.py:15-262) on the HIP path: G(image, attribute), a
TRAINED encoder E(image) -> attribute, and a conditional PatchGAN that judges JOINT pairs, (G(x, y), y) against (x, E(x)).  It is the
one model in which the rating handed to a network is a live, differentiable tensor all the way through: E is trained adversarially
through the discriminator's rating input (loss_E_GAN) and through the generator's (rec_x = G(real_x, E(real_x))), besides the
y -> x -> y cycle.

Same plugin surface as the reference: flags and defaults, the 7 loss names, visual / model names, assertions, and the step order
forward -> D -> G and E together.  Each pair is used once in backward_D (generated side detached) and once in backward_GE; E_GAN has
target False.  Disabled loss terms are the Python float 0.0.

It is WSGANCycleModel (models/wsgan_cycle_model.py: the same flags, networks, cycles, identity term on its branch and generator
names) with a conditional discriminator, one more loss and `--loadSize 128`.

Stated differences from the reference, beyond wsgan_cycle's:
  * forward() and the two discriminator passes of backward_GE() run inside hip.functional.fused_concat_bwd(): the gradient with
    respect to the rating comes from one launch per join (csrc/concat_bwd.hip) -- twice per step with only the rating's gradient
    live, real_x needing none.  PCGAN_CONCATZ_FUSED=0 keeps the chain of copies and channel sums;
  * a torch.distributed run of more than one rank is refused (multi-rank training of this model has not been built).
"""
from .wsgan_cycle_model import WSGANCycleModel
from ..hip import functional as HF


class WSGANBiGANModel(WSGANCycleModel):
    DEFAULT_OVERRIDES = dict(WSGANCycleModel.DEFAULT_OVERRIDES, loadSize=128)   # reference :46-57
    ONE_RANK_REFUSAL = 'pcgan_amd: wsgan_bigan trains on one rank; a run of %d ranks is not supported'
    LOSS_NAMES = ['G_GAN', 'E_GAN', 'G_IP', 'cycle_x', 'cycle_y', 'D_real', 'D_fake']
    CONDITIONAL_D = True    # discriminator of joint pairs: nz = embedding_nc, called D(image, rating)   (:101-103)

    def forward(self):
        with HF.fused_concat_bwd():     # rec_x = G(real_x, fake_y): real_x needs no gradient, only the rating's is formed
            WSGANCycleModel.forward(self)

    def adversarial_terms(self):
        with HF.fused_concat_bwd():
            # (G(y), y) = (fake_x, real_y)
            self.loss_G_GAN = self.criterionGAN(self.judge(self.fake_x, self.real_y), True)
            # (x, E(x)) = (real_x, fake_y): the encoder's adversarial signal is the gradient of D with respect to its rating input
            self.loss_E_GAN = self.criterionGAN(self.judge(self.real_x, self.fake_y), False)
        return [self.loss_G_GAN, self.loss_E_GAN]
