"""Prototypical Contrastive Learning (Li, Zhou, Xiong, Hoi, ICLR 2021) on the HIP path.  The reference has no such trainer: PCL is MoCo (models/moco.py - the
momentum encoder, the queue, the InfoNCE loss, all unchanged) plus a ProtoNCE term.  Once per epoch - the E-step - the momentum encoder's features of the whole
train split are clustered M times (eval_utils.kmeans, ``num_clusters``); the L2-normalised centroids are the prototypes, every prototype gets its own
temperature, the concentration phi of eval_utils.cluster_concentration, and every sample remembers its cluster in each clustering.  A step then pulls each
query to its own prototypes and pushes it from all the others (utils.losses.ProtoNceLoss on csrc/protonce.hip) beside MoCo's loss.

The prototypes, 1 / phi and the label table [M, N] live in device buffers whose addresses never change: the E-step copies into them, a step gathers its rows of
the table by the batch's ``index`` on the device, so one captured graph of the step serves every epoch after the warm-up (and another one the warm-up: the switch
is part of ``graph_key``).  During the first ``warmup_epochs`` epochs the loss is InfoNCE alone, and those epochs are MoCo's bit for bit.

Config block ``pcl: {num_clusters: [..], warmup_epochs, alpha, temperature, niter, nredo, seed}``; at most 8 clusterings, each of at most SSV_KMEANS_MAX_K
clusters and at most as many as the train split has images.  Single-process."""
import torch

from .. import _lib, nn as hnn, ops
from .. import distributed as hdist
from ..utils import eval_utils, losses
from .moco import EncoderModel, MemoryBank, MoCo  # noqa: F401


class PCL(MoCo):
    algo = "pcl"
    graph_safe = True    # MoCo's step plus a gather by the batch's index from the label table and the ProtoNCE launches: device memory only
    graph_inputs = ("aug_1", "aug_2", "index")

    def _build(self, arch):
        if hdist.is_on():
            raise NotImplementedError("PCL is single-process: the prototypes are not replicated across ranks")
        super()._build(arch)                                            # MoCo's modules, in MoCo's order: the same seed gives the same weights
        cfg = dict(self.config.get("pcl") or {})
        self.num_clusters = [int(k) for k in cfg.get("num_clusters", [])]
        n = self._num_train()
        if not 1 <= len(self.num_clusters) <= _lib.PROTO_NCE_MAX_SEGS:
            raise ValueError(f"PCL: pcl.num_clusters must name 1 to {_lib.PROTO_NCE_MAX_SEGS} clusterings (got {self.num_clusters})")
        if any(not 1 <= k <= min(n, _lib.KMEANS_MAX_K) for k in self.num_clusters):
            raise ValueError(f"PCL: every entry of pcl.num_clusters must lie in [1, min({n} train images, {_lib.KMEANS_MAX_K})] (got {self.num_clusters})")
        self.proto_warmup = int(cfg.get("warmup_epochs", 0))
        self.alpha, self.phi_temperature = float(cfg.get("alpha", 10.0)), float(cfg.get("temperature", 0.2))
        self.kmeans_opts = {"niter": int(cfg.get("niter", 20)), "nredo": int(cfg.get("nredo", 1)), "seed": int(cfg.get("seed", 1234))}
        self.seg_end = tuple(sum(self.num_clusters[:s + 1]) for s in range(len(self.num_clusters)))
        dim = self.config["proj_dim"]
        # persistent: their addresses are part of the captured step
        self.prototypes = ops.fill_(torch.empty((self.seg_end[-1], dim), dtype=torch.float32, device=self.device), 0.0)
        self.inv_phi = ops.fill_(torch.empty(self.seg_end[-1], dtype=torch.float32, device=self.device), 1.0)
        self.cluster_labels = torch.zeros((len(self.num_clusters), n), dtype=torch.int32, device=self.device)
        self.proto_loss_fn = losses.ProtoNceLoss(normalize=self.config["loss_fn"].get("normalize", True))
        self.proto_on = False
        self._epoch = 0

    def _num_train(self):
        """Images of the train split: rows of the label table (a trainer built without loaders - benchmarks - counts the placeholders it was given)"""
        return int(getattr(self.train_loader, "shape", (len(self.train_loader),))[0])

    def graph_key(self):
        return super().graph_key() + (bool(self.proto_on),)

    @torch.no_grad()
    def key_features(self):
        """[N, D] on the device: the momentum encoder's L2-normalised embeddings of the train split, row i = sample i"""
        n = self._num_train()
        feats = torch.empty((n, self.config["proj_dim"]), dtype=torch.float32, device=self.device)
        for batch in self.train_loader.eval_batches():
            z = ops.l2norm_fwd(self.key_encoder(batch["img"].to(self.device)).contiguous(), True)[0]
            feats.index_copy_(0, batch["index"].to(self.device), z)
        return feats

    @torch.no_grad()
    def e_step(self):
        """Cluster the momentum features once per entry of ``num_clusters`` and refresh the prototypes, 1 / phi and the label table in place.  The flag of the
        previous epoch's last ProtoNCE call is read here - once per epoch, never per step."""
        ops.check_proto_nce_flag(self.proto_loss_fn.last_flag)
        ops.invalidate_weight_caches()
        feats = self.key_features()
        opts = dict(self.kmeans_opts)
        seed = opts.pop("seed")
        for s, k in enumerate(self.num_clusters):
            run = eval_utils.kmeans(feats, k, seed=seed + s, device=self.device, **opts)
            labels, dist, counts, _ = ops.kmeans_assign(feats, run["centroids"])
            phi = eval_utils.cluster_concentration(dist, labels, counts, alpha=self.alpha, temperature=self.phi_temperature)
            b, e = self.seg_end[s] - k, self.seg_end[s]
            ops.l2norm_fwd(run["centroids"].contiguous(), True, out=self.prototypes[b:e])
            self.inv_phi[b:e].copy_(1.0 / phi)
            self.cluster_labels[s].copy_(labels)
        ops.invalidate_weight_caches()
        self.proto_on = True

    def _run_epoch(self, tag):
        self._epoch += 1
        if self._epoch > self.proto_warmup:
            self.e_step()
        return super()._run_epoch(tag)

    def train_step(self, batch):
        img_1, img_2 = batch["aug_1"].to(self.device), batch["aug_2"].to(self.device)
        with hnn.parallel_views(self.device) as pv:
            with pv.view(0):
                query = self.query_encoder(img_1)
            with pv.view(1):
                with torch.no_grad():
                    keys = self.key_encoder(img_2)
        loss = self.loss_fn(query, keys, self.memory_bank.get_vectors(), self.memory_bank.size)
        if self.proto_on:
            labels = self.cluster_labels.index_select(1, batch["index"].to(self.device))          # [M, B]: gathered on the device
            loss = loss + self.proto_loss_fn(query, self.prototypes, self.inv_phi, labels, self.seg_end)
        loss_now = hnn.early_item(loss)                  # the scalar leaves for the host now; the backward does not wait for it, nor it for the backward
        self.optim.zero_grad()
        loss.backward()
        self.optim.step()
        self.momentum_update()
        self.memory_bank.add_batch(keys)
        return {"loss": loss_now.get()}
