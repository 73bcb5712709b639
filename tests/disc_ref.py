"""Test-side twin of the wsgan_disc step (reference models/wsgan_disc_model.py:162-298) in plain torch, any dtype: resnet / U-Net
generator and conditional PatchGAN of oracle.networks_ref / unet_ref fed with one-hot class labels, the classifier of classifier_ref,
AlexNet identity features, and a plain-torch restatement of the per-class image pool (PoolRef).  Every ReLU / LeakyReLU and max pooling
is a taped one, so DecisionTape.replay works on it.  Pinned to the reference itself by tests/golden/disc_step*.npz and disc_pool.npz
(scripts/make_disc_golden.py, tests/test_disc_oracle_golden.py).

Also the ONE description of the fixture variants -- command lines, seeds, seeded batches, seeded weights -- which the fixture generator,
the CPU test and the GPU test share."""
import os
import random
import sys
from collections import OrderedDict
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import classifier_ref as CR
import unet_ref as U
from oracle import networks_ref as N
from oracle import weights as W
from oracle.step_ref import gan_loss, upsample2d

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
LOSS_NAMES = ['G_GAN', 'G_GAN_cycle', 'G_IP', 'G_L1', 'G_AC', 'G_cycle', 'D_real_right', 'D_real_wrong', 'D_fake', 'AC_real', 'AC_fake']
K = 3                   # classes
REFERENCE_DRAWS = sys.version_info < (3, 11)      # this interpreter's `random` makes the draws the fixtures recorded (see step())
PY_SEED = 777           # Python's global generator is seeded with PY_SEED + it before set_input: the label triple, then the pool's draws
SEED_G, SEED_D, SEED_AC, SEED_IP = 19, 20, 46, 40
# The classifier of the fixture stands for a TRAINED one, which is what --pretrained_model_path_AC names in use: it is not wildly
# confident in a wrong class.  With plain seeded fc weights (and a zero fc bias) the gradient of that one loss term is nearly ALL of the
# generator's gradient: in the float64 twin the share || g - g(lambda_AC = 0) || / || g ||, median over the generator's weight tensors
# of iteration 0, was
#     default 0.992, aux_on_fake_L1 0.994, detach_no_A_GAN 0.999, norm_D_instance 0.993, pool 0.992, unet 0.999
# so the other readers of fake_B -- the discriminator, the second generator pass, the L1 and identity terms -- were invisible in it.
# AC_FC_DAMP shrinks the seeded fc weights of the CHECKPOINT (the reference, the twin and the HIP run all load the same file); at 0.01
# the shares are
#     default 0.087, aux_on_fake_L1 0.064, detach_no_A_GAN 0.221, norm_D_instance 0.087, pool 0.087, unet 0.393
# no resnet variant above a third, so every reader weighs in.  (The U-Net variant's classifier runs at 128 x 128, as in cont_ref.py.)
AC_FC_DAMP = 0.01
GRAD_STRIDE = 997
POOL_PASS = -1          # plan entries, as hip/lib.py has them: pass, store into slot s = 2 s, exchange with slot s = 2 s + 1

# name -> (extra command line, overrides of the twin's options, iterations)
VARIANTS = OrderedDict([
    ('default', ([], {}, 2)),
    ('aux_on_fake_L1', (['--train_aux_on_fake', '--lambda_L1', '0.5'], dict(train_aux_on_fake=True, lambda_L1=0.5), 2)),
    ('detach_no_A_GAN', (['--detach_fake_B', '--lambda_A_GAN', '0'], dict(detach_fake_B=True, lambda_A_GAN=0.0), 2)),
    ('norm_D_instance', (['--norm_D', 'instance'], dict(norm_D='instance'), 2)),
    ('unet', (['--which_model_netG', 'unet', '--fineSize', '128', '--loadSize', '128', '--batchSize', '2', '--fineSize_AC', '128',
               '--fineSize_IP', '128'], dict(netG='unet', fineSize=128, batch=2, fineSize_AC=128, fineSize_IP=128), 2)),
    ('pool', (['--pool_size', '3'], dict(pool_size=3, train_label_pairs=['0 1', '2 1']), 3)),
])
DEFAULTS = dict(netG='resnet_9blocks', fineSize=32, batch=4, fineSize_AC=64, fineSize_IP=64, norm_D='batch', lambda_L1=0.0, lambda_IP=1.0,
                lambda_AC=1.0, lambda_A=0.5, lambda_A_GAN=0.5, train_aux_on_fake=False, detach_fake_B=False, lr=2e-4, lr_AC=2e-4,
                beta1=0.5, identity_preserving_criterion='mse', pool_size=0, train_label_pairs=None, num_classes=K)


def fixture_path(name):
    return os.path.join(GOLD, 'disc_step.npz' if name == 'default' else 'disc_step_%s.npz' % name)


def iterations(name):
    return VARIANTS[name][2]


def options(name):
    o = dict(DEFAULTS)
    o.update(VARIANTS[name][1])
    return SimpleNamespace(**o)


def argv(name, root, ac_path, ip_path, gpu_ids):
    """the training command line of a variant (the reference's parser and this project's take the same one); the `pool` variant's
    label-pair file is written into `root`"""
    base = ['train.py', '--dataroot', root, '--model', 'wsgan_disc', '--name', 'g_disc_' + name, '--checkpoints_dir', root,
            '--gpu_ids', gpu_ids, '--which_model_netG', 'resnet_9blocks', '--which_model_netD', 'n_layers', '--n_layers_D', '3',
            '--ngf', '8', '--ndf', '8', '--fineSize', '32', '--loadSize', '32', '--fineSize_AC', '64', '--fineSize_IP', '64',
            '--batchSize', '4', '--num_classes', str(K), '--embedding_nc', str(K), '--attr_bins', '[10, 30, 50]',
            '--pretrained_model_path_AC', ac_path, '--pretrained_model_path_IP', ip_path, '--display_id', '-1']
    extra = list(VARIANTS[name][0])
    pairs = VARIANTS[name][1].get('train_label_pairs')
    if pairs:
        path = os.path.join(root, 'label_pairs_%s.txt' % name)
        with open(path, 'w') as f:
            f.write('\n'.join(pairs) + '\n')
        extra += ['--train_label_pairs', path]
    return base + extra


def batch(name, it):
    """the seeded input dict of iteration `it` of a variant, as WSGANDiscDataset's loader yields it: one image set per class"""
    o = options(name)
    ret = {}
    for L in range(K):
        ret[L] = W.seeded_tensor((o.batch, 3, o.fineSize, o.fineSize), 900 + 50 * L + it)
        ret['path_%d' % L] = ['c%d' % L] * o.batch
    return ret


def generator_weights(sd, which):
    """seeded weights with the last convolution shrunk so that tanh stays in its linear range (oracle.weights.damp_generator_head)"""
    sd = dict(W.fill_state_dict(sd, SEED_G))
    last = 'model.26.weight' if which.startswith('resnet') else 'model.model.3.weight'
    sd[last] = sd[last] * 0.05
    return sd


def classifier_weights(sd):
    """the classifier's seeded state dict -- the file --pretrained_model_path_AC names -- with its fc weights shrunk by AC_FC_DAMP and a
    zero fc bias (see there)"""
    sd = dict(W.fill_state_dict(sd, SEED_AC))
    sd['model.fc.weight'] = sd['model.fc.weight'] * AC_FC_DAMP
    sd['model.fc.bias'] = torch.zeros_like(sd['model.fc.bias'])
    return sd


# ---- the image pool, restated ------------------------------------------------------------------------------------------------------------
def pool_apply(pool, x, plan):
    """the per-image loop of the reference's ImagePool.query (util/image_pool.py:16-30) for decisions already made: pool (S, ...) is
    updated in place, the returned batch is fresh.  Copies only, so any dtype (integer views included) passes through bit for bit."""
    y = torch.empty_like(x)
    for i, op in enumerate(plan):
        if op < 0:
            y[i] = x[i]
        elif op % 2 == 0:
            pool[op // 2] = x[i]
            y[i] = x[i]
        else:
            y[i] = pool[op // 2].clone()
            pool[op // 2] = x[i]
    return y


class PoolRef:
    """ImagePool with the reference's draws (from Python's global `random`, in its order) and pool_apply as its data path"""

    def __init__(self, pool_size):
        self.pool_size, self.num_imgs, self.images = pool_size, 0, None

    def plan_for(self, n):
        plan = []
        for _ in range(n):
            if self.num_imgs < self.pool_size:
                plan.append(2 * self.num_imgs)
                self.num_imgs += 1
            elif random.uniform(0, 1) > 0.5:
                plan.append(2 * random.randint(0, self.pool_size - 1) + 1)
            else:
                plan.append(POOL_PASS)
        return plan

    def query(self, images, plan=None):
        if self.pool_size == 0:
            return images
        if self.images is None:
            self.images = torch.zeros((self.pool_size,) + tuple(images.shape[1:]), dtype=images.dtype)
        self.last_plan = self.plan_for(images.shape[0]) if plan is None else list(plan)
        return pool_apply(self.images, images.detach(), self.last_plan)


# ---- the step ---------------------------------------------------------------------------------------------------------------------------
class WSGANDiscStepRef:
    """the reference's optimize_parameters(): forward, D, AC, G.  transform_AC / transform_IP are the identity."""

    LOSS_NAMES = LOSS_NAMES

    def __init__(self, netG, netD, netAC, netIP, opt):
        self.opt = opt
        self.netG, self.netD, self.netAC, self.netIP = netG, netD, netAC, netIP
        betas = (opt.beta1, 0.999)
        self.optimizer_G = torch.optim.Adam(netG.parameters(), lr=opt.lr, betas=betas)
        self.optimizer_D = torch.optim.Adam(netD.parameters(), lr=opt.lr, betas=betas)
        self.optimizer_AC = torch.optim.Adam(netAC.parameters(), lr=opt.lr_AC, betas=betas)
        self.dtype = next(netG.parameters()).dtype
        self.one_hot = [torch.eye(K, dtype=self.dtype)[L].view(1, K, 1, 1) for L in range(K)]
        self.fake_B_pool = [PoolRef(opt.pool_size) for _ in range(K)]
        self.current_iter = 0
        self.forced_labels = None       # (label_A, label_B, label_B_not) to use instead of the draw, and a forced pool plan
        self.forced_plan = None
        self.grads = {}

    def sample_label_pairs(self):
        o = self.opt
        if o.train_label_pairs:
            ab = o.train_label_pairs[self.current_iter % len(o.train_label_pairs)].split()
        else:
            ab = random.sample(range(K), 2)
        return int(ab[0]), int(ab[1]), random.sample(sorted(set(range(K)) - set([int(ab[1])])), 1)[0]

    def set_input(self, input):
        o = self.opt
        drawn = self.sample_label_pairs()
        self.label_A, self.label_B, self.label_B_not = drawn if self.forced_labels is None else self.forced_labels
        self.real_A, self.real_B = input[self.label_A].to(self.dtype), input[self.label_B].to(self.dtype)
        self.real_A_IP = upsample2d(self.real_A, o.fineSize_IP)
        self.real_B_AC = upsample2d(self.real_B, o.fineSize_AC)
        self.current_iter += 1

    def labels(self):
        return torch.full((self.real_A.size(0),), self.label_B, dtype=torch.int64)

    def forward(self):
        o = self.opt
        self.fake_B = self.netG(self.real_A, self.one_hot[self.label_B])
        self.fake_B_IP = upsample2d(self.fake_B, o.fineSize_IP)
        self.fake_B_AC = upsample2d(self.fake_B, o.fineSize_AC)
        self.rec_A = self.netG(self.fake_B.detach() if o.detach_fake_B else self.fake_B, self.one_hot[self.label_A])

    def backward_D(self):
        pool = self.fake_B_pool[self.label_B]
        self.fake_B_from_pool = pool.query(self.fake_B.detach(), self.forced_plan).detach()
        self.pool_plan = pool.last_plan if self.opt.pool_size > 0 else []
        self.loss_D_fake = gan_loss(self.netD(self.fake_B_from_pool, self.one_hot[self.label_B]), False)
        self.loss_D_real_right = gan_loss(self.netD(self.real_B, self.one_hot[self.label_B]), True)
        self.loss_D_real_wrong = gan_loss(self.netD(self.real_B, self.one_hot[self.label_B_not]), False)
        self.loss_D = (self.loss_D_fake + (self.loss_D_real_right + self.loss_D_real_wrong) * 0.5) * 0.5
        self.loss_D.backward()

    def backward_AC(self):
        self.loss_AC_real = F.cross_entropy(self.netAC(self.real_B_AC), self.labels())
        if self.opt.train_aux_on_fake:
            self.loss_AC_fake = F.cross_entropy(self.netAC(self.fake_B_AC.detach()), self.labels())
        else:
            self.loss_AC_fake = 0.0
        self.loss_AC = (self.loss_AC_fake + self.loss_AC_real) * 0.5
        self.loss_AC.backward()

    def backward_G(self):
        o = self.opt
        self.loss_G_GAN = gan_loss(self.netD(self.fake_B, self.one_hot[self.label_B]), True)
        self.loss_G_GAN_cycle = gan_loss(self.netD(self.rec_A, self.one_hot[self.label_A]), True) * o.lambda_A_GAN if o.lambda_A_GAN > 0.0 else 0.0
        self.loss_G_L1 = F.l1_loss(self.fake_B, self.real_A) * o.lambda_L1 if o.lambda_L1 > 0.0 else 0.0
        if o.lambda_IP > 0.0:
            feature_A = self.netIP(self.real_A_IP).detach()
            crit = F.mse_loss if o.identity_preserving_criterion.lower() == 'mse' else F.l1_loss
            self.loss_G_IP = crit(self.netIP(self.fake_B_IP), feature_A) * o.lambda_IP
        else:
            self.loss_G_IP = 0.0
        self.loss_G_AC = F.cross_entropy(self.netAC(self.fake_B_AC), self.labels()) * o.lambda_AC if o.lambda_AC > 0.0 else 0.0
        self.loss_G_cycle = F.l1_loss(self.rec_A, self.real_A) * o.lambda_A if o.lambda_A > 0.0 else 0.0
        self.loss_G = self.loss_G_GAN + self.loss_G_IP + self.loss_G_L1 + self.loss_G_AC + self.loss_G_cycle + self.loss_G_GAN_cycle
        self.loss_G.backward()

    @staticmethod
    def _requires_grad(net, flag):
        for p in net.parameters():
            p.requires_grad = flag

    def _grab(self, tag, net):
        self.grads[tag] = {k: (p.grad.detach().clone() if p.grad is not None else None) for k, p in net.named_parameters()}

    def optimize_parameters(self):
        self.forward()
        self._requires_grad(self.netD, True)
        self.optimizer_D.zero_grad()
        self.backward_D()
        self._grab('D', self.netD)
        self.optimizer_D.step()
        self._requires_grad(self.netAC, True)
        self.optimizer_AC.zero_grad()
        self.backward_AC()
        self._grab('AC', self.netAC)
        self.optimizer_AC.step()
        self._requires_grad(self.netD, False)
        self._requires_grad(self.netAC, False)
        self.optimizer_G.zero_grad()
        self.backward_G()
        self._grab('G', self.netG)
        self.optimizer_G.step()

    def losses(self):
        values = {n: getattr(self, 'loss_' + n) for n in self.LOSS_NAMES}
        return {n: float(v.detach() if isinstance(v, torch.Tensor) else v) for n, v in values.items()}


def build_twin(name, dtype=torch.float32, **override):
    """the twin of a fixture variant with the fixture's seeded weights"""
    o = options(name)
    for k, v in override.items():
        setattr(o, k, v)
    if o.netG == 'unet':
        G = U.UnetGeneratorRef(3, 3, K, 7, 8, 'instance')
    else:
        G = N.ResnetGeneratorRef(3, 3, K, 8, 'instance', 9)
    G.load_state_dict(generator_weights(G.state_dict(), o.netG))
    D = N.NLayerDiscriminatorRef(3, K, 8, 3, o.norm_D, True)
    D.load_state_dict(W.fill_state_dict(D.state_dict(), SEED_D))
    AC = CR.ResNetClassifierRef('resnet18', K)
    AC.load_state_dict(classifier_weights(AC.state_dict()))
    IP = N.AlexNetFeatureRef(3, 'None')
    IP.load_state_dict(W.fill_state_dict(IP.state_dict(), SEED_IP))
    for net in (G, D, AC, IP):
        net.to(dtype)
    return WSGANDiscStepRef(G, D, AC, IP, o)


def step(m, name, it, gold=None):
    """one seeded iteration of a twin or of the HIP model.  The fixtures hold the reference's draws under Python <= 3.10; where this
    interpreter's random.sample may pick differently for the same seed (REFERENCE_DRAWS false) and `gold` is given, the label triple and
    the pool's plan are set from the fixture instead of drawn."""
    torch.manual_seed(1234 + it)
    random.seed(PY_SEED + it)
    if gold is not None and not REFERENCE_DRAWS:
        labels = tuple(int(v) for v in gold['it%d/labels' % it])
        plan = [int(v) for v in gold['it%d/pool_plan' % it]] if 'it%d/pool_plan' % it in gold else None
        if isinstance(m, WSGANDiscStepRef):
            m.forced_labels, m.forced_plan = labels, plan
        else:
            m.sample_label_pairs = lambda: labels
            if plan is not None:
                m.fake_B_pool[labels[1]].plan_for = lambda n: list(plan)
    m.set_input(batch(name, it))
    m.optimize_parameters()
