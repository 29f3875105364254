"""W-MSE (Ermolov, Siarohin, Sangineto, Sebe, ICML 2021, "Whitening for Self-Supervised Representation Learning") on the HIP path.  The reference has no such
trainer: the step has the shape of SimCLR's (models/simclr.py) - no negatives, no momentum network, no predictor, no queue - and the loss whitens the projections of
each view inside small random sub-batches (utils.losses.WmseLoss on csrc/whiten.hip) before it compares the positives.

Everything the loss needs per step lives in device memory - the permutation is drawn on the device from a step counter the loss module owns - so the step replays
as a graph.  The whitening's status (a sub-batch whose covariance has no Cholesky factor) is not read back inside the step: such a block yields NaN and the loss
shows it; ``loss_fn.last_info`` keeps the status tensors."""
from .. import nn as hnn
from ..utils import losses, train_utils
from .base import NETWORKS, TwoViewTrainer
from .heads import WmseProjectionHead as ProjectionHead  # noqa: F401


class WMSE(TwoViewTrainer):
    algo = "wmse"
    graph_safe = True    # the permutation's step counter is device memory (WmseLoss.step_dev); permutation, whitening and loss are part of the step and of its graph
    graph_inputs = ("aug_1", "aug_2")

    def _build(self, arch):
        encoder, encoder_dim = NETWORKS[arch].values()
        cfg = self.config
        self.encoder = encoder(**cfg["encoder"]).to(self.device)
        self.proj_head = ProjectionHead(encoder_dim, cfg.get("head_hidden_dim", 1024), cfg["emb_dim"]).to(self.device)
        self.optim = train_utils.get_optimizer(cfg["optimizer"], params=list(self.encoder.parameters()) + list(self.proj_head.parameters()))
        self.loss_fn = losses.WmseLoss(**cfg["loss_fn"]).reset_step(self.device)      # the counter exists before a step is captured

    def _embed(self, img):
        return self.proj_head(self.encoder(img))

    def train_step(self, batch):
        img_1, img_2 = batch["aug_1"].to(self.device), batch["aug_2"].to(self.device)
        with hnn.parallel_views(self.device) as pv:
            with pv.view(0):
                z_1 = self._embed(img_1)
            with pv.view(1):
                z_2 = self._embed(img_2)
        loss = self.loss_fn(z_1, z_2, check=False)
        loss_now = hnn.early_item(loss)                  # the scalar leaves for the host now; the backward does not wait for it, nor it for the backward
        self.optim.zero_grad()
        loss.backward()
        self.optim.step()
        return {"loss": loss_now.get()}

    def _checkpoint_state(self):
        return {"encoder": self.encoder.state_dict(), "proj_head": self.proj_head.state_dict()}

    def _load_state(self, state):
        self.encoder.load_state_dict(state["encoder"])
        self.proj_head.load_state_dict(state["proj_head"])
