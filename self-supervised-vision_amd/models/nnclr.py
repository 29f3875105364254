"""NNCLR (Dwibedi et al., ICCV 2021, "With a Little Help from My Friends") on the HIP path.  The reference has no such trainer: the step has the shape of
SimCLR's (models/simclr.py) with a predictor behind the projector, and one side of every positive pair is replaced by its nearest neighbour in a support
queue of past projections - models.moco.MemoryBank, searched by the fused lookup of csrc/nnlookup.hip inside utils.losses.NnclrLoss.

The queue starts as unit-norm Gaussian rows (seeded; made on the CPU, then uploaded), so the first steps find neighbours of the embeddings' own scale; the
bank's pad rows are zero and lie behind ``queue_size``, which is all the lookup searches.  The first view's projections are pushed AFTER the lookup, so a
sample never finds itself."""
import torch

from .. import nn as hnn
from ..utils import losses, train_utils
from .base import NETWORKS, TwoViewTrainer
from .heads import NnclrPredictionHead as PredictionHead, NnclrProjectionHead as ProjectionHead  # noqa: F401
from .moco import MemoryBank


def seeded_queue(queue_size, dim, seed):
    """[queue_size, dim] fp32 on the CPU: Gaussian rows of unit norm from torch.Generator().manual_seed(seed)"""
    rows = torch.randn(int(queue_size), int(dim), generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float32)
    return rows / rows.norm(dim=1, keepdim=True)


class NNCLR(TwoViewTrainer):
    algo = "nnclr"
    graph_safe = True    # the queue pointer is device memory (MemoryBank); lookup, loss and queue push are part of the step and of its graph
    graph_inputs = ("aug_1", "aug_2")

    def _build(self, arch):
        encoder, encoder_dim = NETWORKS[arch].values()
        cfg = self.config
        dim = cfg["proj_dim"]
        batch = (cfg.get("data") or {}).get("batch_size", 0)             # a trainer built without loaders (benchmarks) names no batch size
        if cfg["queue_size"] < 2 * batch:
            raise ValueError(f"NNCLR: queue_size ({cfg['queue_size']}) must be at least twice the batch size ({batch})")
        self.encoder = encoder(**cfg["encoder"]).to(self.device)
        self.proj_head = ProjectionHead(encoder_dim, cfg.get("proj_hidden_dim", 2048), dim).to(self.device)
        self.pred_head = PredictionHead(dim, cfg.get("pred_hidden_dim", 4096)).to(self.device)
        self.memory_bank = MemoryBank(cfg["queue_size"], dim, self.device)
        self.memory_bank.bank[:self.memory_bank.size].copy_(seeded_queue(cfg["queue_size"], dim, cfg.get("queue_seed", 0)))
        self.optim = train_utils.get_optimizer(
            cfg["optimizer"], params=list(self.encoder.parameters()) + list(self.proj_head.parameters()) + list(self.pred_head.parameters()))
        self.loss_fn = losses.NnclrLoss(**cfg["loss_fn"])

    def _embed(self, img):
        return self.proj_head(self.encoder(img))

    def train_step(self, batch):
        img_1, img_2 = batch["aug_1"].to(self.device), batch["aug_2"].to(self.device)
        with hnn.parallel_views(self.device) as pv:
            with pv.view(0):
                z_1 = self._embed(img_1)
                p_1 = self.pred_head(z_1)
            with pv.view(1):
                z_2 = self._embed(img_2)
                p_2 = self.pred_head(z_2)
        loss = self.loss_fn(z_1, z_2, p_1, p_2, self.memory_bank.get_vectors(), self.memory_bank.size)
        loss_now = hnn.early_item(loss)                  # the scalar leaves for the host now; the backward does not wait for it, nor it for the backward
        self.optim.zero_grad()
        loss.backward()
        self.optim.step()
        self.memory_bank.add_batch(z_1)                  # after the lookup: a sample never finds itself
        return {"loss": loss_now.get()}

    def _checkpoint_state(self):
        return {"encoder": self.encoder.state_dict(), "proj_head": self.proj_head.state_dict(), "pred_head": self.pred_head.state_dict()}

    def _load_state(self, state):
        self.encoder.load_state_dict(state["encoder"])
        self.proj_head.load_state_dict(state["proj_head"])
        self.pred_head.load_state_dict(state["pred_head"])
