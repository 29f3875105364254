"""GPU: the DenseCL trainer above its kernels (tests/test_gpu_dense_nce.py has the kernels): utils.losses.DenseNceLoss against tests/densecl_oracle.py, the
trainer on the synthetic config cut down to 64 train images and batch 16 (resnet18 with the CIFAR stem ends 16 times below the image: 2 x 2 = 4 cells and 64
queries at 32 x 32, 4 x 4 = 16 cells and 256 queries at 64 x 64; the first-step test runs both) - the first step's loss against the oracle on the tensors the step handed its two loss modules and the matching, which heads the two terms reach, both queues after a
step - four steps eager and replayed, the checkpoint, the refused configs, the command line.

The accuracy rule and FACTOR (tests/densecl_oracle.py) are those of tests/test_gpu_dense_nce.py, where FACTOR was measured."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import densecl_oracle as do
from densecl_oracle import FACTOR, FLOOR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITHS = ("bf16x3", "f32")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _holds(what, got, ref64, ref32):
    e, m = do.errs(got, ref64)
    e32, m32 = do.errs(ref32, ref64)
    print(f"{what}: e {e:.3g} (ref32 {e32:.3g})  m {m:.3g} (ref32 {m32:.3g})")
    return e <= FACTOR * e32 + FLOOR and m <= FACTOR * m32 + FLOOR


# ---- the loss module --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("m,d,K", [(70, 128, 640), (33, 36, 31), (256, 64, 48)])
def test_loss_module_against_fp64(dev, m, d, K, arith):
    from ssv_amd import ops
    from ssv_amd.utils import losses
    _, _, pos, bank, _, _ = do.make_case((m, d, K, "plain"))
    g = torch.Generator().manual_seed(m + d)
    z = 3.0 * torch.randn(m, d, generator=g) + 0.5                        # raw embeddings: the module normalises both grids
    keys = 2.0 * torch.randn(m + 3, d, generator=g) + 0.25 * torch.cat([z, z[:3]])
    zd = z.to(dev).requires_grad_(True)
    fn = losses.DenseNceLoss(normalize=True, temperature=0.2)
    with ops.arithmetic(arith):
        loss = fn(zd, keys.to(dev), pos.to(dev), bank.to(dev), K)
        (2.0 * loss).backward()                                            # backward scales what forward formed
    torch.cuda.synchronize()
    assert torch.equal(zd.detach().cpu(), z), "an input was written"
    assert int(fn.last_flag.item()) == 0 and tuple(fn.last_lse.shape) == (m,)
    r64 = do.queue_nce(z, keys, pos, bank, K, 5.0, torch.float64, normalize=True)
    r32 = do.queue_nce(z, keys, pos, bank, K, 5.0, torch.float32, normalize=True)
    assert r64["pos"] < 0.9 and r64["smax"] <= 60.0
    tag = f"loss-m{m}-d{d}[{arith}]"
    assert _holds(f"{tag}.loss", loss.detach().reshape(1), r64["loss"].reshape(1), r32["loss"].reshape(1))
    assert _holds(f"{tag}.lse", fn.last_lse, r64["lse"], r32["lse"])
    assert _holds(f"{tag}.dz", zd.grad, 2.0 * r64["dq"], 2.0 * r32["dq"])


def test_loss_module_leaves_the_flag_to_the_caller(dev):
    from ssv_amd import _lib, ops
    from ssv_amd.utils import losses
    q, keys, pos, bank, K, _ = do.make_case((16, 32, 40, "plain"))
    pos[3] = keys.shape[0]
    fn = losses.DenseNceLoss(True, 0.2)
    fn(q.to(dev), keys.to(dev), pos.to(dev), bank.to(dev), K)              # does not raise: nothing is read here
    with pytest.raises(_lib.SsvError, match="positive"):
        ops.check_queue_nce_flag(fn.last_flag)
    pos[3] = 0
    fn(q.to(dev), keys.to(dev), pos.to(dev), bank.to(dev), K)
    ops.check_queue_nce_flag(fn.last_flag)


# ---- the trainer ------------------------------------------------------------------------------------------------------------------------------------------------
def _config(tmp_path, batch, num_train, num_test, epochs=2, lam=0.5, size=32, name="densecl.yaml", **block):
    import yaml
    cfg = yaml.safe_load(open(os.path.join(ROOT, "self-supervised-vision_amd", "configs", "densecl_r18_32_synthetic.yaml")))
    cfg["epochs"], cfg["eval_every"] = epochs, 1
    cfg["queue_size"] = 32
    cfg["densecl"] = dict({"loss_lambda": lam, "dense_queue_size": 48}, **block)
    cfg["data"]["batch_size"] = batch
    cfg["data"]["synthetic"] = {"num_train": num_train, "num_test": num_test, "image_size": [size, size], "num_classes": 10}
    cfg["data"]["transforms"]["train"]["random_resized_crop"]["size"] = [size, size]
    cfg["data"]["transforms"]["test"]["center_crop"]["size"] = [size, size]
    cfg["linear_eval"].update(epochs=2)
    path = tmp_path / name
    path.write_text(yaml.dump(cfg, sort_keys=False))
    return path


def _trainer(path, output, load=None):
    from ssv_amd import main as cli
    return cli.trainer_class("densecl")(args={"config": str(path), "arch": "resnet18", "algo": "densecl", "task": "train", "output": output, "load": load})


def _spy(t, monkeypatch):
    """Record what a step hands its two loss modules and the matching (clones on the CPU), and what the matching returns"""
    from ssv_amd import ops
    seen = {}
    cpu = lambda x: x.detach().cpu().clone() if torch.is_tensor(x) else x
    t.loss_fn.register_forward_hook(lambda mod, args, out: seen.__setitem__("global", [cpu(a) for a in args]))
    t.dense_loss_fn.register_forward_hook(lambda mod, args, out: seen.__setitem__("dense", [cpu(a) for a in args]))
    real = ops.dense_match

    def match(f1, f2, *a, **k):
        idx, sim = real(f1, f2, *a, **k)
        seen["match"] = [cpu(f1), cpu(f2), cpu(idx), cpu(sim)]
        return idx, sim
    monkeypatch.setattr(ops, "dense_match", match)
    return seen


@pytest.mark.parametrize("size", [32, 64])
def test_first_step_matches_the_oracle_and_both_queues_advance(dev, tmp_path, monkeypatch, size):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("WANDB_MODE", "disabled")
    t = _trainer(_config(tmp_path, 16, 64, 32, size=size), "first")
    side = size // 16
    s = side * side
    assert t.loss_lambda == 0.5 and t.dense_bank.size == 48 and t.memory_bank.size == 32 and t.graph_key() == (0.999, 0.5)
    seen = _spy(t, monkeypatch)
    batch = next(iter(t.train_loader))
    # a first queue that is not empty, so both terms have negatives with a direction (a fresh queue is rows of zeros: tests/test_gpu_dense_nce.py has that case)
    g = torch.Generator().manual_seed(5)
    t.memory_bank.bank.copy_(torch.nn.functional.normalize(torch.randn(t.memory_bank.bank.shape, generator=g), dim=1))
    t.dense_bank.bank.copy_(torch.nn.functional.normalize(torch.randn(t.dense_bank.bank.shape, generator=g), dim=1))
    from ssv_amd import ops
    ops.invalidate_weight_caches()                                          # the first queue is a GEMM operand whose bf16 planes are cached
    loss = t.train_step(batch)["loss"]
    torch.cuda.synchronize()
    q, k, bank, qsize = seen["global"]
    gq, gk, pos, dbank, dsize = seen["dense"]
    f1, f2, idx, sim = seen["match"]
    assert tuple(f1.shape) == (16, side, side, 512) and tuple(q.shape) == (16, 128) and tuple(gq.shape) == (16 * s, 128) == tuple(gk.shape) and (qsize, dsize) == (32, 48)
    assert torch.equal(pos, idx.view(-1)) and pos.dtype == torch.int32
    # the matching on the step's own maps
    ref = do.dense_match(f1.view(16, s, 512), f2.view(16, s, 512))
    j = idx.long() - s * torch.arange(16)[:, None]
    wrong = j != ref["j"]
    excused = wrong & (ref["cos"].max(dim=2).values - ref["cos"].gather(2, j.clamp(0, s - 1)[:, :, None])[:, :, 0] <= do.TIE)
    assert bool((wrong == excused).all()) and int(excused.sum()) <= 2
    # the loss on what the step handed its modules
    args = (q, k, bank, qsize, gq, gk, pos, dbank, dsize, 0.2, 0.5)
    r64, r32 = do.densecl_loss(*args, torch.float64), do.densecl_loss(*args, torch.float32)
    print(f"global {float(r64['global']):.6f} dense {float(r64['dense']):.6f} combined {float(r64['loss']):.6f} got {loss:.6f}")
    assert _holds("trainer.loss", torch.tensor([loss], dtype=torch.float32), r64["loss"].reshape(1), r32["loss"].reshape(1))
    assert int(t.dense_loss_fn.last_flag.item()) == 0
    # both queues advanced by the batch; the second holds the normalised cell means of the key grid
    assert t.memory_bank.ptr == 16 and t.dense_bank.ptr == 16
    want = torch.nn.functional.normalize(gk.double().view(16, s, 128).mean(dim=1), dim=1)
    rows = t.dense_bank.bank[:16].cpu().double()
    assert torch.allclose(rows.norm(dim=1), torch.ones(16, dtype=torch.float64), atol=1e-6) and float((rows - want).abs().max()) <= 1e-6
    assert torch.allclose(t.memory_bank.bank[:16].cpu().double(), torch.nn.functional.normalize(k.double(), dim=1), atol=1e-6)
    assert torch.equal(t.dense_bank.bank[16:48].cpu(), dbank[16:48])        # the rest of the queue is what it was


@pytest.mark.parametrize("lam", [1.0, 0.0])
def test_each_term_reaches_its_own_head(dev, tmp_path, monkeypatch, lam):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("WANDB_MODE", "disabled")
    t = _trainer(_config(tmp_path, 16, 64, 32, lam=lam), f"lam{lam}")
    assert np.isfinite(t.train_step(next(iter(t.train_loader)))["loss"])
    torch.cuda.synchronize()
    enc = t.query_encoder
    gmax = lambda mod: max(float(p.grad.abs().max()) for p in mod.parameters())
    glob, dense, backbone = gmax(enc.proj_head), gmax(enc.dense_head), gmax(enc.encoder.layer4)
    print(f"lambda {lam}: max |grad| proj_head {glob:.3g} dense_head {dense:.3g} layer4 {backbone:.3g}")
    assert backbone > 0.0
    assert (glob == 0.0 and dense > 0.0) if lam == 1.0 else (glob > 0.0 and dense == 0.0)


def test_four_steps_eager_and_replayed(dev, tmp_path):
    """Batch 16: the four losses are finite and bit-equal between SSV_STEP_GRAPH=0 and SSV_STEP_GRAPH=1 (fresh child processes: the switch is read at import; one
    child and one time limit per leg), so are the lse of every step's dense loss; one capture; the flag stays zero and both queue pointers advance on both paths."""
    path = _config(tmp_path, 16, 64, 32)
    runs = {}
    for mode in ("0", "1"):
        env = dict(os.environ, SSV_STEP_GRAPH=mode, WANDB_MODE="disabled")
        out = tmp_path / f"steps_{mode}.pt"
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "densecl_steps_child.py"), str(path), str(out)], cwd=tmp_path, env=env, capture_output=True,
                             text=True, timeout=600)
        assert res.returncode == 0, res.stdout[-2000:] + "\n" + res.stderr[-3000:]
        runs[mode] = torch.load(out)
    eager, graph = runs["0"], runs["1"]
    assert eager["graph"]["replays"] == 0 and graph["graph"]["disabled"] is None and graph["graph"]["replays"] >= 2 and graph["graph"]["captures"] == 1, (eager["graph"], graph["graph"])
    for r in (eager, graph):
        assert all(np.isfinite(v) and v > 0.0 for v in r["losses"]), r["losses"]
        assert r["flags"] == [0, 0, 0, 0] and r["queue_ptr"] == [16, 0, 16, 0] and r["dense_ptr"] == [16, 32, 0, 16]
    assert eager["losses"] == graph["losses"], (eager["losses"], graph["losses"])
    for a, b in zip(eager["lse"], graph["lse"]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_checkpoint_round_trips(dev, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("WANDB_MODE", "disabled")
    path = _config(tmp_path, 16, 64, 32)
    t = _trainer(path, "a")
    batch = next(iter(t.train_loader))
    assert np.isfinite(t.train_step(batch)["loss"])
    assert sorted(t._checkpoint_state()) == ["encoder"] and any(k.startswith("dense_head.") for k in t._checkpoint_state()["encoder"])
    t.save_checkpoint()
    t2 = _trainer(path, "b", load=t.output_dir)
    torch.cuda.synchronize()
    sa, sb = t.query_encoder.state_dict(), t2.query_encoder.state_dict()
    assert list(sa) == list(sb) and len(sa) > 0 and all(torch.equal(sa[k], sb[k]) for k in sa)
    img = batch["img"]
    e1, e2 = t._embed(img), t2._embed(img)
    assert tuple(e1.shape) == (img.shape[0], 128) and torch.equal(e1, e2)      # _embed is the global projection: every evaluation task works unchanged


def test_trainer_refuses_bad_configs_and_process_groups(dev, tmp_path, monkeypatch):
    from ssv_amd import _lib
    from ssv_amd import distributed as hdist
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("WANDB_MODE", "disabled")
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="loss_lambda"):
            _trainer(_config(tmp_path, 16, 64, 32, lam=bad, name="bad.yaml"), "bad")
    with pytest.raises(ValueError, match="dense_queue_size"):
        _trainer(_config(tmp_path, 16, 64, 32, name="bad.yaml", dense_queue_size=0), "bad")
    # 272 x 272 images leave a map of 17 x 17 = 289 cells: above the matching kernel's limit, refused by name
    big = _trainer(_config(tmp_path, 2, 4, 4, size=272, name="big.yaml"), "big")
    with pytest.raises(ValueError, match=f"SSV_DENSE_MATCH_MAX_S = {_lib.DENSE_MATCH_MAX_S}"):
        big.train_step(next(iter(big.train_loader)))
    t = _trainer(_config(tmp_path, 16, 64, 32), "single")
    monkeypatch.setattr(hdist, "is_on", lambda: True)
    with pytest.raises(NotImplementedError):
        t.dense_loss_fn(torch.zeros(16, 128, device=dev), torch.zeros(16, 128, device=dev), torch.zeros(16, dtype=torch.int32, device=dev), t.dense_bank.bank, 48)
    with pytest.raises(NotImplementedError):
        t._build("resnet18")


# ---- the command line -------------------------------------------------------------------------------------------------------------------------------------------
def test_main_trains_densecl(tmp_path, monkeypatch):
    from ssv_amd import main as cli
    path = _config(tmp_path, 16, 32, 80, epochs=1)                          # one epoch of two steps
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("WANDB_MODE", "disabled")
    model = cli.main(["-c", str(path), "-a", "densecl", "-m", "resnet18", "-t", "train", "-o", "run"])
    out = tmp_path / "outputs" / "densecl" / "resnet18" / "run"
    log = (out / "trainlogs.txt").read_text()
    assert "[TRAIN] Epoch    1/   1 [loss]" in log and "[VALID] Epoch    1/   1 [accuracy]" in log and (out / "best_model.pt").exists()
    torch.cuda.synchronize()
    assert torch.isfinite(model.optim.arena.data).all()
    assert int(model.dense_loss_fn.last_flag.item()) == 0 and model.dense_bank.ptr == 32 and model.memory_bank.ptr == 0
    state = torch.load(out / "best_model.pt", map_location="cpu")
    assert sorted(state) == ["encoder"] and "dense_head.layer2.weight" in state["encoder"]
