"""Dense Contrastive Learning (Wang, Zhang, Shen, Kong, Li, CVPR 2021) on the HIP path.  The reference has no such trainer: DenseCL is MoCo (models/moco.py - the
momentum encoder, the queue, the InfoNCE loss, all unchanged) plus one term that acts on the final feature map.  Every cell of the query view's map is projected by
a dense head (models.heads.DenseProjectionHead), matched to the cell of the key view whose BACKBONE feature is most similar (ops.dense_match on the two maps, no
gradient), and pulled to that cell's key embedding and pushed from a second queue, which holds the per-image means of past key grids
(utils.losses.DenseNceLoss on csrc/densecl.hip):

    loss = (1 - loss_lambda) * MocoLoss(q, k, queue) + loss_lambda * DenseNceLoss(q_grid, k_grid, match, dense queue)

One bridged module per encoder runs the backbone once and yields both projections packed as the rows of one matrix ([B + B * cells, D]: the global projections,
then the grid), and leaves the backbone map for the matching.  Everything a step touches lives in device memory, so the step is replayed as one graph like MoCo's.

Config block ``densecl: {loss_lambda: 0.5, dense_queue_size: <queue_size>}``; a feature map of more than SSV_DENSE_MATCH_MAX_S (256) cells is refused.
Single-process."""
import torch

from .. import _lib, nn as hnn, ops
from .. import distributed as hdist
from ..utils import losses
from .heads import DenseProjectionHead
from .moco import EncoderModel, MemoryBank, MoCo


def _map_rows(tape, fmap):
    """The feature map [B, H, W, C] as rows [B * H * W, C]: the same memory, a second consumer of the map beside the pooling"""
    t = hnn._tensor(fmap)
    rows = t.view(-1, t.shape[-1])
    if tape is not None:
        tape.record((fmap,), rows, lambda dy, ex: (hnn._accum(ex[0], dy.view(t.shape)),))
    return rows


def _pack_rows(tape, a, b):
    """[rows of a; rows of b]: the one output a bridged module has"""
    na = a.shape[0]
    out = torch.empty((na + b.shape[0], a.shape[1]), dtype=torch.float32, device=a.device)
    out[:na].copy_(a)
    out[na:].copy_(b)
    if tape is not None:
        tape.record((a, b), out, lambda dy, ex: (hnn._accum(ex[0], dy[:na]), hnn._accum(ex[1], dy[na:])))
    return out


class DenseEncoderModel(EncoderModel):
    """MoCo's encoder and head with the dense head behind them (built in that order: the first two draw MoCo's weights at the same seed).  forward(img) returns
    [B + B * cells, D]: rows [0, B) the global projection (MoCo's: Linear on the pooled map), rows [B, ...) the dense grid, image by image, cell by cell.
    ``last_map`` is the backbone map [B, H', W', C] of the last forward (no gradient: the matching reads it)."""

    def __init__(self, encoder, encoder_dim, projection_dim):
        super().__init__(encoder, encoder_dim, projection_dim)
        self.dense_head = DenseProjectionHead(encoder_dim, projection_dim)
        object.__setattr__(self, "last_map", None)
        object.__setattr__(self, "global_only", False)

    def embed(self, x):
        """The global projection alone [B, D] (evaluation: the dense head does not run)"""
        object.__setattr__(self, "global_only", True)
        try:
            return self(x)
        finally:
            object.__setattr__(self, "global_only", False)

    def _run(self, tape, x):
        if self.global_only:
            return super()._run(tape, x)
        fmap = self.encoder._feature_map(tape, x)
        glob = self.proj_head._run(tape, hnn.global_avgpool(tape, fmap))         # ReLU(pooled features) == pooled features (models/moco.py)
        rows = _map_rows(tape, fmap)
        object.__setattr__(self, "last_map", hnn._tensor(fmap))
        return _pack_rows(tape, glob, self.dense_head._run(tape, rows))


class DenseCL(MoCo):
    algo = "densecl"
    graph_safe = True    # MoCo's step plus the matching, the dense loss and a second queue push: device memory only
    graph_inputs = ("aug_1", "aug_2")
    encoder_model = DenseEncoderModel

    def _build(self, arch):
        if hdist.is_on():
            raise NotImplementedError("DenseCL is single-process: the dense queue is not replicated across ranks")
        cfg = dict(self.config.get("densecl") or {})
        self.loss_lambda = float(cfg.get("loss_lambda", 0.5))
        if not 0.0 <= self.loss_lambda <= 1.0:
            raise ValueError(f"DenseCL: densecl.loss_lambda must lie in [0, 1] (got {self.loss_lambda})")
        dense_queue = int(cfg.get("dense_queue_size", self.config["queue_size"]))
        if dense_queue < 1:
            raise ValueError(f"DenseCL: densecl.dense_queue_size must be at least 1 (got {dense_queue})")
        super()._build(arch)                                            # MoCo's modules in MoCo's order, each encoder module with its dense head behind it
        self.dense_bank = MemoryBank(dense_queue, self.config["proj_dim"], self.device)
        self.dense_loss_fn = losses.DenseNceLoss(**self.config["loss_fn"])

    def _embed(self, img):
        return self.query_encoder.embed(img)

    def graph_key(self):
        return super().graph_key() + (float(self.loss_lambda),)

    def _run_epoch(self, tag):
        meter = super()._run_epoch(tag)
        ops.check_queue_nce_flag(self.dense_loss_fn.last_flag)          # once per epoch, never per step
        return meter

    def train_step(self, batch):
        img_1, img_2 = batch["aug_1"].to(self.device), batch["aug_2"].to(self.device)
        b = img_1.shape[0]
        with hnn.parallel_views(self.device) as pv:
            with pv.view(0):
                out_q = self.query_encoder(img_1)
            with pv.view(1):
                with torch.no_grad():
                    out_k = self.key_encoder(img_2)
        map_q, map_k = self.query_encoder.last_map, self.key_encoder.last_map
        cells = map_q.shape[1] * map_q.shape[2]
        if cells > _lib.DENSE_MATCH_MAX_S:
            raise ValueError(f"DenseCL: the final feature map has {cells} cells per image, above SSV_DENSE_MATCH_MAX_S = {_lib.DENSE_MATCH_MAX_S} (use smaller images)")
        query, grid_q = out_q[:b], out_q[b:]
        keys, grid_k = out_k[:b], out_k[b:]
        match, _ = ops.dense_match(map_q, map_k)                        # [B, cells] rows of grid_k
        loss = (1.0 - self.loss_lambda) * self.loss_fn(query, keys, self.memory_bank.get_vectors(), self.memory_bank.size) \
            + self.loss_lambda * self.dense_loss_fn(grid_q, grid_k, match.view(-1), self.dense_bank.get_vectors(), self.dense_bank.size)
        loss_now = hnn.early_item(loss)                  # the scalar leaves for the host now; the backward does not wait for it, nor it for the backward
        self.optim.zero_grad()
        loss.backward()
        self.optim.step()
        self.momentum_update()
        self.memory_bank.add_batch(keys)
        self.dense_bank.add_batch(ops.gap_fwd(grid_k.contiguous().view(b, cells, 1, -1)))       # the per-image mean of the key grid; the push normalises
        return {"loss": loss_now.get()}
