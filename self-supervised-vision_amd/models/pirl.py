"""PIRL on the HIP path - drop-in for the reference trainer (models/pirl.py:22-140).

Kept from the reference: one memory-bank row per SAMPLE, zero at start, filled by one no-grad pass over the un-augmented images (train-mode
BatchNorm, so the running statistics move) and then following the image features by momentum without re-normalisation; the jigsaw branch runs
the encoder once per patch - each patch its own BatchNorm batch, x offsets outside y offsets, after the full image - and concatenates the patch
embeddings in a random order in front of g_proj_head_final; a step draws randperm(data_size) for the negatives, then randperm(P) for that order,
from the host generator, so a seeded run draws what the reference draws.

What differs is where things live: the bank is device memory ([N, D] fp32), the loss reads its rows BY INDEX inside the kernel (ops.pirl_loss: no
gathered copy of positives or negatives, no B x K logits in memory), the update is one launch behind the loss on the same stream (the loss sees the
old rows, like the reference), the patches are cut by one launch into dense batches, and the negative filter is one vectorised isin instead of an
O(N B) Python loop.  Per step the host sends the K negative indices and the patch order; the batch indices come back once for the filter."""
import torch

from .. import distributed as hdist, nn as hnn, ops
from ..utils import losses, train_utils
from .base import NETWORKS, TwoViewTrainer
from .heads import _fresh_linear


def sample_negatives(data_size, exclude, k):
    """The first k entries of torch.randperm(data_size) (global CPU generator) that are not in ``exclude``: models/pirl.py:44-46 without the
    per-element loop.  Fewer than k rows left: all of them, like the reference's slice."""
    perm = torch.randperm(int(data_size))
    keep = ~torch.isin(perm, torch.as_tensor(exclude, dtype=torch.long).cpu().reshape(-1))
    return perm[keep][:int(k)].contiguous()


class MemoryBank:
    """models/pirl.py:22-46 with the rows in device memory.  ``indices`` are int64 device tensors, distinct within one call."""

    def __init__(self, data_size, feature_size, momentum=0.5, num_negatives=1000, device=None):
        self.size = self.data_size = int(data_size)
        self.m, self.num_negatives = float(momentum), int(num_negatives)
        self.bank = ops.fill_(torch.empty((self.size, int(feature_size)), dtype=torch.float32, device=device), 0.0)

    def initialize_vectors(self, indices, vectors):
        ops.bank_momentum_update(self.bank, indices, vectors.detach().contiguous(), 0.0)       # rows are zero: 0 * row + the unit vector

    def update_vectors(self, indices, new_vectors):
        ops.bank_momentum_update(self.bank, indices, new_vectors.detach().contiguous(), self.m)

    def get_vectors(self):
        return self.bank

    def negative_indices(self, exclude_idx):
        return sample_negatives(self.data_size, exclude_idx, self.num_negatives)


class EncoderModel(hnn.HipModule):
    """encoder + the image head f and the two jigsaw heads g (created in the reference's order: same init draws, same state_dict keys)."""

    def __init__(self, encoder, encoder_dim, projection_dim, patch_size, num_patches):
        super().__init__()
        self.encoder = encoder
        self.patch_size, self.num_patches = int(patch_size), int(num_patches)
        self.f_proj_head = _fresh_linear(encoder_dim, projection_dim)
        self.g_proj_head_initial = _fresh_linear(encoder_dim, projection_dim)
        self.g_proj_head_final = _fresh_linear(projection_dim * num_patches, projection_dim)
        self._patch_branch = False

    def _prepare_input(self, x):
        return self.encoder._prepare_input(x)

    def _run(self, tape, x):
        head = self.g_proj_head_initial if self._patch_branch else self.f_proj_head
        return head._run(tape, self.encoder._run(tape, x))

    def embed_patch(self, patch):
        """g_proj_head_initial(encoder(patch)) for one batch of patches."""
        self._patch_branch = True
        try:
            return hnn.HipModule.forward(self, patch)
        finally:
            self._patch_branch = False

    def patch_features(self, patching_imgs, order=None):
        """The jigsaw branch: one encoder pass per patch in the reference's patch order, concatenated in ``order`` (default: a fresh
        torch.randperm, drawn after the passes like the reference does)."""
        cut = ops.patch_split(patching_imgs, self.patch_size)
        if cut.shape[0] != self.num_patches:
            raise ValueError(f"patch_size {self.patch_size} cuts {tuple(patching_imgs.shape[2:])} images into {cut.shape[0]} patches, num_patches says {self.num_patches}")
        per_patch = [self.embed_patch(cut[p]) for p in range(cut.shape[0])]
        order = torch.randperm(len(per_patch)) if order is None else order
        return self.g_proj_head_final(torch.cat([per_patch[int(i)] for i in order], 1))

    def forward(self, normal_imgs, patching_imgs=None):
        image_features = hnn.HipModule.forward(self, normal_imgs)
        if patching_imgs is None:
            return image_features
        return image_features, self.patch_features(patching_imgs)


class PIRL(TwoViewTrainer):
    algo = "pirl"
    graph_safe = False   # two host draws per step (negatives, patch order)

    def _build(self, arch):
        if hdist.is_on():
            raise NotImplementedError("data-parallel PIRL is not built: the memory bank is per process")
        encoder, encoder_dim = NETWORKS[arch].values()
        cfg = self.config
        size = getattr(getattr(self.train_loader, "train_tf", None), "size", None)
        if size is not None and (size[0] % cfg["patch_size"] or size[1] % cfg["patch_size"]
                                 or (size[0] // cfg["patch_size"]) * (size[1] // cfg["patch_size"]) != cfg["num_patches"]):
            raise ValueError(f"num_patches {cfg['num_patches']} is not ({size[0]} / {cfg['patch_size']}) * ({size[1]} / {cfg['patch_size']})")
        self.model = EncoderModel(encoder(**cfg["encoder"]), encoder_dim, cfg["proj_dim"], cfg["patch_size"], cfg["num_patches"]).to(self.device)
        self.memory_bank = MemoryBank(self.train_loader.shape[0], cfg["proj_dim"], cfg["momentum"], cfg["num_negatives"], device=self.device)
        self.initialize_memory_vectors()
        self.optim = train_utils.get_optimizer(cfg["optimizer"], params=self.model.parameters())
        self.loss_fn = losses.PirlLoss(**cfg["loss_fn"])

    @torch.no_grad()
    def initialize_memory_vectors(self):
        self.logger.print("Initializing memory bank", mode="info")
        for batch in self.train_loader.eval_batches():
            self.memory_bank.initialize_vectors(batch["index"].to(self.device), self.model(batch["img"].to(self.device)))

    def _embed(self, img):
        return self.model(img)

    def train_step(self, batch):
        index = batch["index"]
        normal_imgs, patching_imgs = batch["aug_1"].to(self.device), batch["aug_2"].to(self.device)
        negatives = self.memory_bank.negative_indices(index).to(self.device)                   # first host draw
        index = index.to(self.device)
        img_features, patch_features = self.model(normal_imgs, patching_imgs)                  # second host draw inside (the patch order)
        loss = self.loss_fn(img_features, patch_features, self.memory_bank.get_vectors(), index, negatives, check=False)
        loss_now = hnn.early_item(loss)                  # the scalar leaves for the host now; the backward does not wait for it, nor it for the backward
        self.memory_bank.update_vectors(index, img_features)                                   # behind the loss kernels on this stream: they saw the old rows
        self.optim.zero_grad()
        loss.backward()
        self.optim.step()
        value = loss_now.get()
        ops.check_pirl_flag(self.loss_fn.last_flag)
        return {"loss": value}

    def _checkpoint_state(self):
        return {"encoder": self.model.state_dict()}

    def _load_state(self, state):
        self.model.load_state_dict(state["encoder"])
