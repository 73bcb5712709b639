"""ImagePool -- the reference's history of generated images (util/image_pool.py) with the images kept in ONE device tensor and a query
served by ONE kernel launch per lib.POOL_PLAN_MAX images (ops.pool_exchange, csrc/image_pool.hip) instead of a host loop of unsqueeze /
clone / cat per image.

The random decisions are the reference's, drawn from Python's global `random` in its order: while the pool is filling an image is stored
and returned with no draw; once it is full `random.uniform(0, 1)` is drawn per image and `random.randint(0, pool_size - 1)` only if it
came out above 0.5.  After `random.seed(k)` the pool therefore hands back what the reference's would.  `plan_for(n)` makes the draws
alone, so a test can inspect a plan or inject its own through `exchange`."""
import random

import torch

from ..hip import lib as _L
from ..hip import ops


class ImagePool():
    def __init__(self, pool_size):
        self.pool_size = pool_size
        if self.pool_size > 0:
            self.num_imgs = 0
            self.images = None          # [pool_size, C, H, W] on the device, allocated by the first query

    def plan_for(self, n):
        """the decisions for the next n images (advances the fill count and the global random state), as plan entries of
        ops.pool_exchange: slot `num_imgs` is stored into while the pool fills, then pass / exchange with a random slot"""
        plan = []
        for _ in range(n):
            if self.num_imgs < self.pool_size:
                plan.append(_L.pool_store(self.num_imgs))
                self.num_imgs = self.num_imgs + 1
            elif random.uniform(0, 1) > 0.5:
                plan.append(_L.pool_swap(random.randint(0, self.pool_size - 1)))     # randint is inclusive
            else:
                plan.append(_L.POOL_PASS)
        return plan

    def exchange(self, images, plan):
        """carry out `plan` for the batch `images`; returns the batch the caller receives (fresh, detached)"""
        images = images.detach()
        if not images.is_contiguous():
            images = images.contiguous()
        self._check(images)
        if self.images is None:
            self.images = torch.zeros((self.pool_size,) + tuple(images.shape[1:]), dtype=images.dtype, device=images.device)
        return ops.pool_exchange(self.images, images, plan)

    def _check(self, images):
        if self.images is not None and (images.shape[1:] != self.images.shape[1:] or images.dtype != self.images.dtype):
            raise RuntimeError('pcgan_amd: ImagePool holds %s images of %s, queried with %s of %s'
                               % (self.images.dtype, tuple(self.images.shape[1:]), images.dtype, tuple(images.shape[1:])))

    def query(self, images):
        if self.pool_size == 0:
            return images
        self._check(images)                 # before any draw is made
        return self.exchange(images, self.plan_for(int(images.shape[0])))
