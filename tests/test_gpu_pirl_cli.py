"""GPU: `main.py -a pirl` end to end on the synthetic data set - train, validate, checkpoint, then get_features from that checkpoint."""
import os

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_main_pirl_trains_and_extracts_features(tmp_path, monkeypatch):
    from ssv_amd import main as cli
    cfg = yaml.safe_load(open(os.path.join(ROOT, "self-supervised-vision_amd", "configs", "pirl.yaml")))
    cfg["epochs"], cfg["eval_every"] = 2, 1
    cfg["data"]["batch_size"] = 16
    cfg["data"]["synthetic"] = {"num_train": 80, "num_test": 48, "image_size": [32, 32], "num_classes": 10}
    cfg["linear_eval"]["epochs"] = 2
    cfg["num_negatives"] = 30
    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.dump(cfg, sort_keys=False))
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("WANDB_MODE", "disabled")
    model = cli.main(["-c", str(path), "-a", "pirl", "-m", "resnet18", "-t", "train", "-o", "run"])
    out = tmp_path / "outputs" / "pirl" / "resnet18" / "run"
    log = (out / "trainlogs.txt").read_text()
    assert "[TRAIN] Epoch    2/   2 [loss]" in log and "[VALID] Epoch    2/   2 [accuracy]" in log and (out / "best_model.pt").exists()
    state = torch.load(out / "best_model.pt", map_location="cpu")["encoder"]
    assert list(state)[0] == "encoder.conv1.weight" and tuple(state["g_proj_head_final.weight"].shape) == (128, 4 * 128)
    assert np.isfinite(model.optim.arena.data.cpu().numpy()).all()
    assert model.memory_bank.bank.shape == (80, 128)
    norms = model.memory_bank.bank.norm(dim=1).cpu().numpy()
    assert (norms > 0).all() and (norms <= 1.0).all(), (norms.min(), norms.max())      # momentum mixtures of unit vectors: inside the unit ball
    feats = cli.main(["-c", str(path), "-a", "pirl", "-m", "resnet18", "-t", "get_features", "-o", "feats", "-l", str(out)])
    fvecs = np.load(feats.output_dir + "/test_fvecs.npy")
    assert fvecs.shape == (48, 128) and np.isfinite(fvecs).all()
    np.testing.assert_allclose(np.linalg.norm(fvecs, axis=1), 1.0, rtol=1e-4)
