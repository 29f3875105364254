#!/usr/bin/env python3
"""Generate tests/golden/pirl_level.npz by running THE REFERENCE ITSELF (models/pirl.py, utils/losses.py:92-117), like gen_golden.py does for
the other algorithms:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_pirl.py

Inputs are seeded CPU tensors defined once in tests/pirl_oracle.py (the tests regenerate them; they are not stored).  The trainer is built with
``object.__new__`` and wired as PIRL.__init__ does (model, memory bank, initialize_memory_vectors, optimizer), without dataloaders / wandb.  It runs
twice - in fp32, and from the same initial weights and inputs in fp64: the distance between the two is the reference's own rounding error on this
configuration and defines the tolerances of the trainer tests.  The archive is written with fixed zip timestamps: regenerating it gives the same bytes.
"""
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import gen_golden as gg            # noqa: E402
import pirl_oracle as po           # noqa: E402


def loss_cases(ref_losses, out):
    for tag, b, d, k, n, normalize, temperature, weight, seed in po.LOSS_CASES:
        img, patch, bank, pos, neg = po.loss_case_inputs(b, d, k, n, seed)
        img.requires_grad_(), patch.requires_grad_()
        loss = ref_losses.PirlLoss(normalize=normalize, temperature=temperature, loss_weight=weight)(img, patch, bank[pos], bank[neg])
        loss.backward()
        out[f"loss_{tag}"], out[f"loss_{tag}_dimg"], out[f"loss_{tag}_dpatch"] = np.float64(loss.item()), img.grad.numpy(), patch.grad.numpy()


def bank_case(ref_pirl, out):
    mb = ref_pirl.MemoryBank(40, 32, momentum=0.5, num_negatives=5)
    (i0, v0), (i1, v1), (i2, v2) = po.bank_case_inputs()
    mb.initialize_vectors(i0, v0)
    mb.update_vectors(i1, v1)
    mb.update_vectors(i2, v2)
    out["bank_case"] = mb.bank.numpy().copy()


def trainer(ref_pirl, ref_losses, ref_tu, out, double):
    cfg, sfx = po.TRAINER, "_f64" if double else ""
    fn, dim = ref_pirl.NETWORKS[cfg["arch"]].values()
    torch.manual_seed(420)
    m = object.__new__(ref_pirl.PIRL)
    m.device = torch.device("cpu")
    m.logger = types.SimpleNamespace(print=lambda *a, **k: None)
    m.model = ref_pirl.EncoderModel(fn(reduce_bottom_conv=cfg["reduce_bottom_conv"]), dim, cfg["proj_dim"], cfg["patch_size"], cfg["num_patches"])
    m.memory_bank = ref_pirl.MemoryBank(cfg["data_size"], cfg["proj_dim"], cfg["momentum"], cfg["num_negatives"])
    cast = (lambda t: t.double()) if double else (lambda t: t)
    if double:
        m.model.double()
        m.memory_bank.bank = m.memory_bank.bank.double()
    else:
        out["init_keys"], out["init_sums"] = gg.state_checksums(m.model.state_dict())
    m.train_loader = [{"index": b["index"], "img": cast(b["img"])} for b in po.init_batches()]
    m.initialize_memory_vectors()
    if not double:
        out["bank_init"] = m.memory_bank.bank.numpy().copy()
        out["after_init_keys"], out["after_init_sums"] = gg.state_checksums(m.model.state_dict())
    m.optim = ref_tu.get_optimizer({"name": "sgd", "lr": cfg["lr"], "weight_decay": cfg["weight_decay"]}, params=m.model.parameters())
    m.loss_fn = ref_losses.PirlLoss(normalize=cfg["normalize"], temperature=cfg["temperature"], loss_weight=cfg["loss_weight"])
    losses, negatives, perms = [], [], []
    real_randperm = torch.randperm
    for s in range(po.STEPS):
        batch = po.step_batch(s)
        drawn = []

        def recording(*a, **k):
            drawn.append(real_randperm(*a, **k))
            return drawn[-1]
        torch.manual_seed(po.step_seed(s))
        torch.randperm = recording
        try:
            losses.append(m.train_step({"index": batch["index"], "aug_1": cast(batch["aug_1"]), "aug_2": cast(batch["aug_2"])})["loss"])
        finally:
            torch.randperm = real_randperm
        assert len(drawn) == 2 and drawn[0].numel() == cfg["data_size"] and drawn[1].numel() == cfg["num_patches"], [d.shape for d in drawn]
        own = set(batch["index"].tolist())
        negatives.append([i for i in drawn[0].tolist() if i not in own][:cfg["num_negatives"]])
        perms.append(drawn[1].tolist())
    out["losses" + sfx] = np.array(losses, dtype=np.float64)
    out["bank_final" + sfx] = m.memory_bank.bank.numpy().copy()
    if not double:
        out["negatives"], out["patch_perms"] = np.array(negatives, dtype=np.int64), np.array(perms, dtype=np.int64)
        out["final_keys"], out["final_sums"] = gg.state_checksums(m.model.state_dict())
    else:
        assert negatives == out["negatives"].tolist() and perms == out["patch_perms"].tolist()         # both runs drew the same indices


def write_npz(path, arrays):
    """np.savez_compressed with constant member timestamps."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def main():
    sys.path.insert(0, gg.REF)
    gg._stub_modules()
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    from models import pirl as ref_pirl
    from utils import losses as ref_losses, train_utils as ref_tu
    out = {}
    loss_cases(ref_losses, out)
    bank_case(ref_pirl, out)
    trainer(ref_pirl, ref_losses, ref_tu, out, double=False)
    trainer(ref_pirl, ref_losses, ref_tu, out, double=True)
    write_npz(os.path.join(HERE, "pirl_level.npz"), out)
    print("pirl_level:", {t[0]: float(out[f"loss_{t[0]}"]) for t in po.LOSS_CASES}, out["losses"], out["losses_f64"],
          float(np.abs(out["bank_final"] - out["bank_final_f64"]).max()))


if __name__ == "__main__":
    main()
