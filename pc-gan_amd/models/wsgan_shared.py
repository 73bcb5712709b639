"""What the baseline models share (wsgan_cycle, wsgan_bigan, wsgan_cont, wsgan_disc; wsgan_emb has a stream structure of its own and
stands apart): WSGANBase between BaseModel and the four, and WSGANPairModel under the two CGAN baselines.  No model lives here, and
the file name does not end in `_model`, so the registry does not list it.

WSGANBase: the flag tables of a class applied to the parser, the construction helpers, the AlexNet identity term, one update of one
or more networks, the visuals, the test-time end of set_input() and test().  Three settings per model:
  SOURCE            name of the attribute that holds the input image ('real_A' | 'real_x');
  IP_ON_BRANCH      the identity term is issued on hip.ops.branch('IP'), beside the discriminator's passes (wsgan_cycle, wsgan_bigan),
                    or on the main stream (wsgan_cont, wsgan_disc).  Launch order follows from it, so the fixtures pin each value;
  ONE_RANK_REFUSAL  None: data parallelism is one process per GPU + RCCL all-reduce of the flat gradient buffers (instead of the
                    reference's nn.DataParallel), replicas start from rank 0's weights.  A text: multi-rank training of the model has
                    not been built -- a run of more than one rank is refused with it at construction AND the model issues no
                    collective at all (parallel.is_distributed() can be true in a world of one rank: PCGAN_FORCE_COLLECTIVES).

WSGANPairModel: forward -> D -> auxiliary net -> G of the two CGAN baselines.  Stated differences from the reference, both models:
  * when fineSize_IP equals the auxiliary net's fineSize, one upsample2d(fake_B) feeds both the identity net and the auxiliary net;
  * fake_B, rec_A and that shared resized image reach their consumers through hip.functional.fan_out, so the gradients coming back
    are summed by one kernel launch each (csrc/grad_fanin.hip) where autograd would chain binary adds.  PCGAN_FANOUT=0 (read once,
    when this module is imported) hands the tensors on unchanged and autograd accumulates as before.
Everything a pair model issues runs on the main stream (no branches); the library's parameter-gradient side stream is as elsewhere.
"""
import os
from collections import OrderedDict

import numpy as np
import torch

from . import networks
from .base_model import BaseModel
from ..hip import functional as HF
from ..hip import ops as hip_ops
from ..hip import parallel
from ..hip.optim import FusedAdam
from ..util.util import upsample2d

_FANOUT = os.environ.get('PCGAN_FANOUT', '1') != '0'


def _fan(x, n):
    """x for n consumers: n aliases whose gradients one launch sums (or x itself n times: PCGAN_FANOUT=0, one consumer, no graph)"""
    if not _FANOUT or n < 2 or not x.requires_grad:
        return [x] * n
    return list(HF.fan_out(x, n))


def sum_terms(terms):
    """((t0 + t1) + t2) + ...: a loss summed left to right as the reference writes it, the floats 0.0 of disabled terms included"""
    total = terms[0]
    for t in terms[1:]:
        total = total + t
    return total


class WSGANBase(BaseModel):
    COMMON_FLAGS, TRAIN_FLAGS, DEFAULT_OVERRIDES = [], [], {}      # each model's own tables: [(flag, add_argument keywords)]
    SOURCE = 'real_A'
    IP_ON_BRANCH = False
    ONE_RANK_REFUSAL = None
    AUX = 'E'       # the third network beside G and D ('E' | 'AC'): net<AUX>, optimizer_<AUX>, transform_<AUX>

    def name(self):
        return type(self).__name__

    @classmethod
    def modify_commandline_options(cls, parser, is_train=True):
        for flag, kw in cls.COMMON_FLAGS + (cls.TRAIN_FLAGS if is_train else []):
            parser.add_argument(flag, **kw)
        parser.set_defaults(**cls.DEFAULT_OVERRIDES)
        return parser

    # ------------------------------------------------------------------ construction
    def initialize(self, opt):
        BaseModel.initialize(self, opt)
        assert opt.input_nc == opt.output_nc
        if self.ONE_RANK_REFUSAL and parallel.is_distributed() and torch.distributed.get_world_size() > 1:
            raise NotImplementedError(self.ONE_RANK_REFUSAL % torch.distributed.get_world_size())
        self.attr_bins = opt.attr_bins

    def define_G(self, **kw):
        o = self.opt
        return networks.define_G(o.input_nc, o.output_nc, o.embedding_nc, o.ngf, which_model_netG=o.which_model_netG, norm=o.norm_G,
                                 nl=o.nl, dropout=o.dropout, init_type=o.init_type, gpu_ids=self.gpu_ids, upsample=o.upsample, **kw)

    def define_D(self, nz, **kw):
        """nz = 0: unconditional, called D(image); nz > 0: called D(image, condition of nz channels)"""
        o = self.opt
        return networks.define_D(o.output_nc, nz, o.ndf, o.which_model_netD, o.n_layers_D, o.norm_D, o.no_lsgan, o.init_type,
                                 num_Ds=o.num_Ds, gpu_ids=self.gpu_ids, **kw)

    def define_IP(self):
        """the AlexNet identity net with its pretrained weights (not saved, never trained)"""
        net = networks.define_IP(self.opt.which_model_netIP, self.opt.input_nc, self.gpu_ids)
        getattr(net, 'module', net).load_pretrained(self.opt.pretrained_model_path_IP)
        return net

    def define_criteria(self):
        o = self.opt
        self.criterionGAN = networks.GANLoss(use_lsgan=not o.no_lsgan, tensor=self.Tensor)
        self.criterionL1 = networks.L1Loss()
        crit = o.identity_preserving_criterion.lower()
        if crit == 'mse':
            self.criterionIP = networks.MSELoss()
        elif crit == 'l1':
            self.criterionIP = networks.L1Loss()
        else:
            raise NotImplementedError('Not Implemented')
        self.criterionCycle = networks.L1Loss()

    def define_optimizers(self, built, lr_aux):
        """optimizer_<X> = FusedAdam over net<X> for every X of `built`, in that order; G and D at --lr, the third net at lr_aux.
        self.optimizers is the reference's order in all four models: G, D, the third"""
        o = self.opt
        if not self.ONE_RANK_REFUSAL:
            for net in (self.netG, self.netD, getattr(self, 'net' + self.AUX), self.netIP):
                parallel.broadcast_parameters(net)
        for x in built:
            adam = FusedAdam(getattr(self, 'net' + x).parameters(), lr=lr_aux if x == self.AUX else o.lr, betas=(o.beta1, 0.999))
            setattr(self, 'optimizer_' + x, adam)
        self.optimizers = [self.optimizer_G, self.optimizer_D, getattr(self, 'optimizer_' + self.AUX)]
        self.set_requires_grad(self.netIP, False)   # no optimizer in the reference either: its gradients are unused

    def define_attr_normalize(self):
        o = self.opt
        self.attr_mean, self.attr_std = o.attr_mean, o.attr_std
        mean, std = o.attr_mean[0], o.attr_std[0]
        self.attr_normalize = lambda x: (x - mean) / std
        if o.display_visuals:
            self.pre_generate_embeddings()

    def pre_generate_embeddings(self):
        arr = np.array(self.opt.attr_bins).reshape(len(self.opt.attr_bins), 1, 1, 1, 1)
        self.fixed_embeddings = [self.attr_normalize(torch.Tensor(arr[i]).to(self.device)) for i in range(arr.shape[0])]

    def define_transforms(self):
        self.transform_IP = networks.Normalize((0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010))
        setattr(self, 'transform_' + self.AUX, networks.Normalize((0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010)))

    # ------------------------------------------------------------------ the step
    def end_set_input(self, input):
        """what every set_input() ends with: at test time the image and, where the loader has one, B's attribute; the counters"""
        if not self.isTrain:
            setattr(self, self.SOURCE, self.to_act(input['A']))
            self.image_paths = input['A_paths']
            if 'B_attr' in input:
                self.set_attr_B(input['B_attr'].to(self.device, non_blocking=True))
                self.image_paths = input['B_paths']
        self.current_iter += 1
        self.current_batch_size = int(getattr(self, self.SOURCE).size(0))

    def set_attr_B(self, attr):
        self.attr_B = attr

    def test(self):
        return

    def sample_from_label(self, label):
        attr_B = torch.Tensor([self.attr_bins[label]]).reshape(1, 1, 1, 1).to(self.device)
        return self.netG(getattr(self, self.SOURCE), self.attr_normalize(attr_B))

    def identity_term(self, real_IP, fake_IP):
        """loss_G_IP = criterionIP(netIP(fake), netIP(real)) * lambda_IP, the features of `real` without a graph; the float 0.0 when
        the term is off.  Returns the branch it was issued on (IP_ON_BRANCH; otherwise one that is off and the term is in stream
        order): the caller join()s it with loss_G_IP before it sums the losses"""
        o = self.opt
        b = hip_ops.branch('IP', enabled=self.IP_ON_BRANCH and o.lambda_IP > 0.0)
        if o.lambda_IP > 0.0:
            with b:
                with torch.no_grad():
                    feature_A = self.netIP(self.transform_IP(real_IP))
                self.loss_G_IP = self.criterionIP(self.netIP(self.transform_IP(fake_IP)), feature_A) * o.lambda_IP
        else:
            self.loss_G_IP = 0.0
        return b

    def update(self, names, backward, requires_grad):
        """one update of the networks `names`: requires_grad ({network name: flag}, in order) set as given, the gradients zeroed,
        backward(), then all gradient syncs, all steps, all replica checks"""
        for x, flag in requires_grad.items():
            self.set_requires_grad(getattr(self, 'net' + x), flag)
        optimizers = [getattr(self, 'optimizer_' + x) for x in names]
        for optimizer in optimizers:
            optimizer.zero_grad()
        backward()
        if not self.ONE_RANK_REFUSAL:
            for optimizer in optimizers:
                parallel.sync_gradients(optimizer)
        for optimizer in optimizers:
            optimizer.step()
        if not self.ONE_RANK_REFUSAL:
            for x, optimizer in zip(names, optimizers):
                parallel.ddp_check(optimizer, x)

    def embeddings_to_show(self):
        return self.fixed_embeddings

    def get_current_visuals(self):
        self.set_requires_grad(self.netG, False)
        ret = OrderedDict()
        for name in self.visual_names:
            if isinstance(name, str):
                ret[name] = getattr(self, name)
        if self.opt.display_visuals:
            for L, embedding in enumerate(self.embeddings_to_show()):
                ret['attr_' + str(L)] = self.netG(getattr(self, self.SOURCE)[0:1, ...], embedding)
        self.set_requires_grad(self.netG, True)
        return ret


class WSGANPairModel(WSGANBase):
    """G(real_A, condition of B) -> fake_B -> G(fake_B, condition of A) -> rec_A against a conditional PatchGAN, with an auxiliary net
    (AUX: the regressor 'E' | the classifier 'AC') that is trained inside the step on real_B and judges fake_B in the G update.
    A model supplies conditioning(), aux_loss(image), backward_D() and its names:
      AUX_LOSS   'AR' | 'AC': --lambda_<AUX_LOSS>, loss_<AUX_LOSS>_real, loss_<AUX_LOSS>_fake;
      G_SUM      the terms of the generator's loss in the order the reference sums them; the auxiliary term's name is G_AUX_TERM."""
    AUX_LOSS = G_AUX_TERM = None
    G_SUM = ()

    def define_pair_nets(self):
        """G and, for training, D (conditional: nz = embedding_nc) and the identity net -- in this order"""
        self.netG = self.define_G(size=self.opt.fineSize)
        if self.isTrain:
            self.netD = self.define_D(self.opt.embedding_nc, size=self.opt.fineSize)
            self.netIP = self.define_IP()

    def load_aux(self, path):
        """the auxiliary net's whole state dict, strict (what regression.py / classification.py write)"""
        if not self.opt.continue_train and path:
            net = getattr(self, 'net' + self.AUX)
            getattr(net, 'module', net).load_state_dict(torch.load(path, map_location='cpu'), strict=True)

    def forward(self):
        o = self.opt
        fine_aux = getattr(o, 'fineSize_' + self.AUX)
        self.embedding_A, self.embedding_B = self.conditioning()
        self.fake_B = self.netG(self.real_A, self.embedding_B)
        # who reads fake_B in backward_G: the discriminator join, the second generator pass, the L1 term and the resize(s) feeding
        # the identity net and the auxiliary net -- one alias each, in this order (the order of the gradient sum)
        want_ip, want_aux = o.lambda_IP > 0.0, getattr(o, 'lambda_' + self.AUX_LOSS) > 0.0
        shared = want_ip and want_aux and o.fineSize_IP == fine_aux
        readers = ['D'] + ([] if o.detach_fake_B else ['G2']) + (['L1'] if o.lambda_L1 > 0.0 else [])
        readers += ['big'] if shared else (['IP'] if want_ip else []) + (['aux'] if want_aux else [])
        fb = dict(zip(readers, _fan(self.fake_B, len(readers))))
        self._fake_B_D, self._fake_B_L1 = fb['D'], fb.get('L1')
        if shared:
            self.fake_B_IP, fake_B_aux = _fan(upsample2d(fb['big'], fine_aux), 2)
        else:
            # a term that is switched off reads nothing; --train_aux_on_fake still needs the (detached) auxiliary input
            self.fake_B_IP = upsample2d(fb['IP'], o.fineSize_IP) if want_ip else None
            fake_B_aux = None
            if want_aux or o.train_aux_on_fake:
                fake_B_aux = upsample2d(fb['aux'] if want_aux else self.fake_B.detach(), fine_aux)
        setattr(self, 'fake_B_' + self.AUX, fake_B_aux)
        self.rec_A = self.netG(self.fake_B.detach() if o.detach_fake_B else fb['G2'], self.embedding_A)
        # rec_A is read by the discriminator (--lambda_A_GAN) and by the cycle L1 (--lambda_A)
        readers = (['D'] if o.lambda_A_GAN > 0.0 else []) + (['cycle'] if o.lambda_A > 0.0 else [])
        ra = dict(zip(readers, _fan(self.rec_A, len(readers))))
        self._rec_A_D, self._rec_A_cycle = ra.get('D'), ra.get('cycle')

    def backward_aux(self):
        real = self.aux_loss(getattr(self, 'real_B_' + self.AUX))
        fake = self.aux_loss(getattr(self, 'fake_B_' + self.AUX).detach()) if self.opt.train_aux_on_fake else 0.0
        setattr(self, 'loss_%s_real' % self.AUX_LOSS, real)
        setattr(self, 'loss_%s_fake' % self.AUX_LOSS, fake)
        loss = (fake + real) * 0.5
        setattr(self, 'loss_' + self.AUX_LOSS, loss)
        loss.backward()

    def backward_G(self):
        o = self.opt
        lambda_aux = getattr(o, 'lambda_' + self.AUX_LOSS)
        self.loss_G_GAN = self.criterionGAN(self.netD(self._fake_B_D, self.embedding_B), True)
        if o.lambda_A_GAN > 0.0:
            self.loss_G_GAN_cycle = self.criterionGAN(self.netD(self._rec_A_D, self.embedding_A), True) * o.lambda_A_GAN
        else:
            self.loss_G_GAN_cycle = 0.0
        self.loss_G_L1 = self.criterionL1(self._fake_B_L1, self.real_A) * o.lambda_L1 if o.lambda_L1 > 0.0 else 0.0
        b_ip = self.identity_term(self.real_A_IP, self.fake_B_IP)
        aux = self.aux_loss(getattr(self, 'fake_B_' + self.AUX)) * lambda_aux if lambda_aux > 0.0 else 0.0
        setattr(self, 'loss_' + self.G_AUX_TERM, aux)
        self.loss_G_cycle = self.criterionCycle(self._rec_A_cycle, self.real_A) * o.lambda_A if o.lambda_A > 0.0 else 0.0
        b_ip.join(self.loss_G_IP)
        self.loss_G = sum_terms([getattr(self, 'loss_' + term) for term in self.G_SUM])
        self.loss_G.backward()

    def optimize_parameters(self):
        self.forward()
        self.update(['D'], self.backward_D, {'D': True})
        self.update([self.AUX], self.backward_aux, {self.AUX: True})
        self.update(['G'], self.backward_G, {'D': False, self.AUX: False})
