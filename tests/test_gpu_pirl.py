"""GPU: PIRL on the HIP path - the gathered NCE loss kernel, the memory-bank update, the jigsaw cut, the encoder at patch size and the trainer -
against the reference's fixture (tests/golden/pirl_level.npz, tests/golden/gen_golden_pirl.py) and torch on the CPU."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pirl_oracle as po           # noqa: E402

pytestmark = pytest.mark.gpu

LOSS_RTOL, GRAD_RTOL, GRAD_ATOL = 1e-5, 1e-3, 2e-7          # the MoCo loss kernel's bounds (tests/test_gpu_siblings.py)
BANK_RTOL, BANK_ATOL = 2e-3, 5e-4                           # the MoCo queue's bound after three steps (tests/test_gpu_siblings.py)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _loss(dev, img, patch, bank, pos, neg, normalize, temperature, weight, splits=None):
    from ssv_amd import ops
    loss, dimg, dpatch, flag = ops.pirl_loss(bank.to(dev), pos.to(dev), neg.to(dev), img.to(dev), patch.to(dev), normalize, 1.0 / temperature, weight, splits=splits)
    ops.check_pirl_flag(flag)
    return float(loss.item()), dimg.cpu(), dpatch.cpu()


def test_loss_kernel_matches_the_reference(dev, golden):
    from ssv_amd.utils import losses
    g = golden["pirl_level"]
    for tag, b, d, k, n, normalize, temperature, weight, seed in po.LOSS_CASES:
        img, patch, bank, pos, neg = po.loss_case_inputs(b, d, k, n, seed)
        zi, zp = img.to(dev).requires_grad_(), patch.to(dev).requires_grad_()
        loss = losses.PirlLoss(normalize, temperature, weight)(zi, zp, bank.to(dev), pos.to(dev), neg.to(dev))
        loss.backward()
        print(tag, loss.item(), float(g[f"loss_{tag}"]), float((zi.grad.cpu() - torch.tensor(g[f"loss_{tag}_dimg"])).abs().max()),
              float((zp.grad.cpu() - torch.tensor(g[f"loss_{tag}_dpatch"])).abs().max()))
        np.testing.assert_allclose(loss.item(), g[f"loss_{tag}"], rtol=LOSS_RTOL, err_msg=tag)
        np.testing.assert_allclose(zi.grad.cpu().numpy(), g[f"loss_{tag}_dimg"], rtol=GRAD_RTOL, atol=GRAD_ATOL, err_msg=tag)
        np.testing.assert_allclose(zp.grad.cpu().numpy(), g[f"loss_{tag}_dpatch"], rtol=GRAD_RTOL, atol=GRAD_ATOL, err_msg=tag)
        # backward scales the stored gradients by the incoming one
        zi2, zp2 = img.to(dev).requires_grad_(), patch.to(dev).requires_grad_()
        (3.0 * losses.PirlLoss(normalize, temperature, weight)(zi2, zp2, bank.to(dev), pos.to(dev), neg.to(dev))).backward()
        np.testing.assert_allclose(zi2.grad.cpu().numpy(), 3.0 * zi.grad.cpu().numpy(), rtol=1e-6, atol=1e-12)


def _fp_reference(img, patch, bank, pos, neg, normalize, temperature, weight, dtype):
    zi, zp = img.detach().to(dtype).clone().requires_grad_(), patch.detach().to(dtype).clone().requires_grad_()
    b = bank.to(dtype)
    loss = po.pirl_loss(zi, zp, b[pos], b[neg], normalize, temperature, weight)
    loss.backward()
    return float(loss.item()), zi.grad, zp.grad


@pytest.mark.parametrize("b,d,k,n", [(1024, 128, 32003, 200000), (3, 20, 5, 8)])
def test_loss_kernel_at_sizes_the_fixture_cannot_hold(dev, monkeypatch, b, d, k, n):
    """K split across workgroups, rows gathered from a large bank, tails in B, K and D: against torch fp64 on the CPU.  Bound: 3 x the error torch fp32 on
    the CPU makes against that fp64 result on the same inputs (the fp64-envelope convention), the fixture test's rtol / atol as floor."""
    from ssv_amd import ops
    img, patch, bank, pos, neg = po.loss_case_inputs(b, d, k, n, 2200 + b)
    assert neg.numel() == k
    normalize, temperature, weight = True, 0.07, 0.3
    l64, di64, dp64 = _fp_reference(img, patch, bank, pos, neg, normalize, temperature, weight, torch.float64)
    l32, di32, dp32 = _fp_reference(img, patch, bank, pos, neg, normalize, temperature, weight, torch.float32)
    loss_bound = max(3 * abs(l32 - l64), LOSS_RTOL * abs(l64))

    def grad_bound(g32, g64):
        return torch.maximum(3 * (g32.double() - g64).abs().max(), GRAD_ATOL + GRAD_RTOL * g64.abs())

    def check(got, what):
        loss, dimg, dpatch = got
        e_i, e_p = (dimg.double() - di64).abs(), (dpatch.double() - dp64).abs()
        print(what, "loss", loss, l64, "err", abs(loss - l64), "bound", loss_bound, "| dimg err", float(e_i.max()), "fp32 cpu err", float((di32.double() - di64).abs().max()),
              "| dpatch err", float(e_p.max()), "fp32 cpu err", float((dp32.double() - dp64).abs().max()))
        assert abs(loss - l64) <= loss_bound, (what, loss, l64, loss_bound)
        assert bool((e_i <= grad_bound(di32, di64)).all()) and bool((e_p <= grad_bound(dp32, dp64)).all()), (what, float(e_i.max()), float(e_p.max()))

    first = _loss(dev, img, patch, bank, pos, neg, normalize, temperature, weight)
    check(first, "default splits")
    again = _loss(dev, img, patch, bank, pos, neg, normalize, temperature, weight)
    assert first[0] == again[0] and torch.equal(first[1], again[1]) and torch.equal(first[2], again[2])          # bit-identical
    for forced in (1, 64):                                        # the K split forced to one run and to its maximum (the library clamps it to the tile count)
        monkeypatch.setattr(ops, "PIRL_SPLITS", forced)
        assert ops.pirl_splits() == forced
        check(_loss(dev, img, patch, bank, pos, neg, normalize, temperature, weight), f"ops.PIRL_SPLITS = {forced}")


@pytest.mark.parametrize("d", [4, 36, 256, 512])
def test_loss_kernel_takes_every_width_up_to_512(dev, d):
    """The narrowest and the widest rows (512: the staged block fills 64 KiB of LDS exactly, without the padding column), and a width that is a multiple of
    4 but not of 8 - against torch fp64 on the CPU, same bounds as the large-shape test."""
    b, k, n = 40, 70, 300
    img, patch, bank, pos, neg = po.loss_case_inputs(b, d, k, n, 2700 + d)
    for normalize in (True, False):
        l64, di64, dp64 = _fp_reference(img, patch, bank, pos, neg, normalize, 0.5, 0.5, torch.float64)
        l32, di32, dp32 = _fp_reference(img, patch, bank, pos, neg, normalize, 0.5, 0.5, torch.float32)
        loss, dimg, dpatch = _loss(dev, img, patch, bank, pos, neg, normalize, 0.5, 0.5)
        e_i, e_p = (dimg.double() - di64).abs(), (dpatch.double() - dp64).abs()
        print(d, normalize, "loss err", abs(loss - l64), "fp32 cpu", abs(l32 - l64), "grad err", float(e_i.max()), float(e_p.max()),
              "fp32 cpu", float((di32.double() - di64).abs().max()), float((dp32.double() - dp64).abs().max()))
        assert abs(loss - l64) <= max(3 * abs(l32 - l64), LOSS_RTOL * abs(l64))
        assert bool((e_i <= torch.maximum(3 * (di32.double() - di64).abs().max(), GRAD_ATOL + GRAD_RTOL * di64.abs())).all())
        assert bool((e_p <= torch.maximum(3 * (dp32.double() - dp64).abs().max(), GRAD_ATOL + GRAD_RTOL * dp64.abs())).all())


def test_loss_kernel_refuses_what_it_cannot_take(dev):
    from ssv_amd import _lib, ops
    img, patch, bank, pos, neg = po.loss_case_inputs(4, 18, 6, 16, 2300)               # D = 18: not a multiple of 4
    with pytest.raises(_lib.SsvError):
        ops.pirl_loss(bank.to(dev), pos.to(dev), neg.to(dev), img.to(dev), patch.to(dev), True, 1.0, 0.5)


def test_one_index_outside_the_bank_raises(dev):
    """pos_index[0] = N: the row is left out, nothing is read out of range, the flag word becomes SsvError.  Run once."""
    from ssv_amd import _lib
    from ssv_amd.utils import losses
    img, patch, bank, pos, neg = po.loss_case_inputs(8, 32, 12, 40, 2400)
    pos[0] = 40
    with pytest.raises(_lib.SsvError, match="outside the memory bank"):
        losses.PirlLoss(True, 0.07, 0.5)(img.to(dev), patch.to(dev), bank.to(dev), pos.to(dev), neg.to(dev))


def test_bank_update_matches_the_reference(dev, golden):
    from ssv_amd.models.pirl import MemoryBank
    g = golden["pirl_level"]
    mb = MemoryBank(40, 32, momentum=0.5, num_negatives=5, device=dev)
    (i0, v0), (i1, v1), (i2, v2) = po.bank_case_inputs()
    mb.initialize_vectors(i0.to(dev), v0.to(dev))
    mb.update_vectors(i1.to(dev), v1.to(dev))
    before = mb.bank.clone()
    mb.update_vectors(i2.to(dev), v2.to(dev))                     # row 3 of this call is all zero
    got = mb.bank.cpu()
    assert bool(torch.isfinite(got).all())
    np.testing.assert_allclose(got[i2[3]].numpy(), 0.5 * before[i2[3]].cpu().numpy(), rtol=1e-6, atol=1e-7)      # the zero feature only shrinks its row
    np.testing.assert_allclose(got.numpy(), g["bank_case"], rtol=1e-6, atol=1e-7)
    untouched = torch.ones(40, dtype=torch.bool)
    untouched[i2] = False
    assert torch.equal(got[untouched], before.cpu()[untouched])                        # rows not indexed: bit-unchanged


@pytest.mark.parametrize("ps", [16, 8])
@pytest.mark.parametrize("channels_last", [True, False])
def test_patch_split_is_the_reference_slices(dev, ps, channels_last):
    from ssv_amd import ops
    x = po.randn(2500 + ps, 5, 3, 32, 32)
    xd = x.to(dev).contiguous(memory_format=torch.channels_last) if channels_last else x.to(dev)
    got = ops.patch_split(xd, ps)
    want = po.patches(x, ps)
    assert got.shape == (len(want), 5, 3, ps, ps)
    for p, w in enumerate(want):
        assert got[p].is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(got[p].cpu(), w), p


def test_encoder_at_patch_size_matches_the_cpu(dev):
    """resnet18 (reduce_bottom_conv) on 16 x 16 inputs: 2 x 2 maps in layer3, 1 x 1 in layer4 - the shapes PIRL's patch branch runs.  Forward and backward
    against oracle.nets.resnet_forward in fp64, held to the fp32 CPU evaluation's own distance like the other architecture checks of tests/test_gpu_step.py."""
    from ssv_amd.networks import resnet
    torch.manual_seed(420)
    net = resnet.resnet18(reduce_bottom_conv=True).to(dev)
    x, dy = po.randn(2600, 16, 3, 16, 16), po.randn(2601, 16, 512)
    y = net(x.to(dev))
    y.backward(dy.to(dev))

    def cpu(dtype):
        torch.manual_seed(420)
        p = {k: (v.to(dtype) if v.dtype.is_floating_point else v) for k, v in oracle.init_resnet("resnet18", True).items()}
        for k, v in p.items():
            if v.dtype.is_floating_point and "running" not in k:
                v.requires_grad_(True)
        out = oracle.resnet_forward(p, x.to(dtype), "resnet18", True)
        out.backward(dy.to(dtype))
        return p, out.detach()
    p64, y64 = cpu(torch.float64)
    p32, y32 = cpu(torch.float32)
    e_cpu, e_hip = float((y32.double() - y64).abs().max()), float((y.detach().cpu().double() - y64).abs().max())
    errs = {name: float((p.grad.cpu().double() - p64[name].grad).norm() / (p64[name].grad.norm() + 1e-30)) for name, p in net.named_parameters()}
    cpu_err = np.array([float((p32[k].grad.double() - p64[k].grad).norm() / (p64[k].grad.norm() + 1e-30)) for k in errs])
    vals = np.array(list(errs.values()))
    print("features", e_hip, e_cpu, "gradients median", float(np.median(vals)), float(np.median(cpu_err)), "max", float(vals.max()), float(cpu_err.max()))
    assert e_hip <= 3 * e_cpu + 1e-5, (e_hip, e_cpu)
    assert np.median(vals) <= 3 * np.median(cpu_err) + 1e-4 and vals.max() <= 3 * cpu_err.max() + 1e-3, \
        (float(np.median(vals)), float(np.median(cpu_err)), float(vals.max()), float(cpu_err.max()))


class _Loader:
    """What PIRL._build reads of a loader: the data set's shape and the in-order evaluation batches."""
    shape = (po.TRAINER["data_size"], 32, 32, 3)

    def __len__(self):
        return po.TRAINER["data_size"] // po.BATCH

    def eval_batches(self):
        return iter(po.init_batches())


def _trainer(dev):
    from ssv_amd.models.pirl import PIRL
    from ssv_amd.utils import train_utils
    c = po.TRAINER
    t = object.__new__(PIRL)
    t.config = {"epochs": 1000, "encoder": {"reduce_bottom_conv": c["reduce_bottom_conv"]}, "scheduler": {"name": "cosine", "warmup_epochs": 0},
                "proj_dim": c["proj_dim"], "patch_size": c["patch_size"], "num_patches": c["num_patches"], "num_negatives": c["num_negatives"],
                "momentum": c["momentum"], "optimizer": {"name": "sgd", "lr": c["lr"], "weight_decay": c["weight_decay"]},
                "loss_fn": {"normalize": c["normalize"], "temperature": c["temperature"], "loss_weight": c["loss_weight"]}}
    t.device, t.train_loader, t.logger = dev, _Loader(), types.SimpleNamespace(print=lambda *a, **k: None)
    return t


def test_trainer_matches_the_reference(dev, golden):
    """Init checksums exact; the bank after initialize_memory_vectors at the MoCo bank bound; three seeded steps: losses and the final bank within
    max(floor, 3 x the reference's own fp32-vs-fp64 distance), both read from the fixture."""
    g = golden["pirl_level"]
    t = _trainer(dev)
    torch.manual_seed(420)
    made = {}
    build = type(t).initialize_memory_vectors

    def checked_init(self):                                       # the reference initialises the bank inside its constructor: look at the weights before it
        made["sd"] = {k: v.detach().cpu().clone() for k, v in self.model.state_dict().items()}
        build(self)
    t.initialize_memory_vectors = types.MethodType(checked_init, t)
    t._build(po.TRAINER["arch"])
    for k, ref in zip(g["init_keys"], g["init_sums"]):
        np.testing.assert_allclose(np.array(oracle.tensor_checksum(made["sd"][str(k)].contiguous())), ref, rtol=1e-12, atol=0, err_msg=str(k))
    assert [k for k in made["sd"] if made["sd"][k].dtype.is_floating_point] == [str(k) for k in g["init_keys"]]
    bank = t.memory_bank.bank.cpu().numpy()
    print("bank after init: max err", float(np.abs(bank - g["bank_init"]).max()))
    np.testing.assert_allclose(bank, g["bank_init"], rtol=BANK_RTOL, atol=BANK_ATOL)
    sd = t.model.state_dict()
    for k, ref in zip(g["after_init_keys"], g["after_init_sums"]):                     # the no-grad pass moved the BatchNorm running statistics
        if "running_" in str(k):
            np.testing.assert_allclose(oracle.tensor_checksum(sd[str(k)].cpu().contiguous())[1], ref[1], rtol=5e-3, err_msg=str(k))
    losses = []
    for s in range(po.STEPS):
        torch.manual_seed(po.step_seed(s))
        losses.append(t.train_step(po.step_batch(s))["loss"])
    gap = np.abs(g["losses"] - g["losses_f64"])
    bound = np.maximum(LOSS_RTOL * np.abs(g["losses_f64"]), 3 * gap)
    print("losses", losses, "reference", g["losses"].tolist(), "fp64", g["losses_f64"].tolist(), "bound", bound.tolist())
    assert np.isfinite(losses).all()
    for s in range(po.STEPS):
        assert abs(losses[s] - g["losses"][s]) <= bound[s], (s, losses[s], float(g["losses"][s]), float(bound[s]))
    bank = t.memory_bank.bank.cpu().numpy()
    bank_gap = 3 * float(np.abs(g["bank_final"] - g["bank_final_f64"]).max())
    err = np.abs(bank - g["bank_final"])
    print("final bank: max err", float(err.max()), "3 x fp32-vs-fp64", bank_gap)
    assert bool((err <= np.maximum(BANK_ATOL + BANK_RTOL * np.abs(g["bank_final"]), bank_gap)).all()), float(err.max())


def test_num_patches_must_match_the_cut(dev):
    t = _trainer(dev)
    t.config["num_patches"] = 9
    torch.manual_seed(420)
    t._build(po.TRAINER["arch"])
    with pytest.raises(ValueError, match="num_patches"):
        t.train_step(po.step_batch(0))
