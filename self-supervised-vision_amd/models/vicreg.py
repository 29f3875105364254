"""VICReg (Bardes, Ponce, LeCun 2022) on the HIP path.  The reference has no such trainer: the step has the shape of Barlow Twins' (models/barlow.py), the
projector is Barlow's without its final L2 normalisation, the loss is utils.losses.VicregLoss."""
from .. import nn as hnn
from ..utils import losses, train_utils
from .base import NETWORKS, TwoViewTrainer
from .heads import VicregProjectionHead as ProjectionHead  # noqa: F401


class VICReg(TwoViewTrainer):
    algo = "vicreg"
    graph_safe = True    # the step holds no per-step host state: inputs, loss, BatchNorm statistics, optimizer state are device memory
    graph_inputs = ("aug_1", "aug_2")

    def _build(self, arch):
        encoder, encoder_dim = NETWORKS[arch].values()
        self.encoder = encoder(**self.config["encoder"]).to(self.device)
        self.proj_head = ProjectionHead(encoder_dim, self.config["proj_dim"]).to(self.device)
        self.optim = train_utils.get_optimizer(
            self.config["optimizer"], params=list(self.encoder.parameters()) + list(self.proj_head.parameters()))
        self.loss_fn = losses.VicregLoss(**self.config["loss_fn"])

    def _embed(self, img):
        return self.proj_head(self.encoder(img))

    def train_step(self, batch):
        img_1, img_2 = batch["aug_1"].to(self.device), batch["aug_2"].to(self.device)
        with hnn.parallel_views(self.device) as pv:
            with pv.view(0):
                z_1 = self._embed(img_1)
            with pv.view(1):
                z_2 = self._embed(img_2)
        loss = self.loss_fn(z_1, z_2)
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
