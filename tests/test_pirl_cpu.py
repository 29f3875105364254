"""CPU: PIRL's host side - the CLI entry, the negative sampler's draw order, the configuration file - and the CPU restatement
(tests/pirl_oracle.py) against the reference's fixture (tests/golden/pirl_level.npz)."""
import os
import sys

import numpy as np
import pytest
import torch
import yaml

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pirl_oracle as po           # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cli_resolves_pirl_and_still_refuses_the_unbuilt_algorithms():
    from ssv_amd import main as cli
    from ssv_amd.models.pirl import PIRL
    assert cli.trainer_class("pirl") is PIRL and PIRL.algo == "pirl" and PIRL.graph_safe is False
    for algo in ("swav", "sela", "deep_cluster"):
        with pytest.raises(NotImplementedError):
            cli.trainer_class(algo)
    assert cli.parse(["-c", "x.yaml", "-a", "pirl", "-m", "resnet18", "-t", "train"])["algo"] == "pirl"


def test_sample_negatives_draws_what_the_reference_drew(golden):
    from ssv_amd.models.pirl import sample_negatives
    g = golden["pirl_level"]
    c = po.TRAINER
    for s in range(po.STEPS):
        index = po.step_batch(s)["index"]
        torch.manual_seed(po.step_seed(s))
        got = sample_negatives(c["data_size"], index, c["num_negatives"])
        assert got.dtype == torch.int64 and got.tolist() == g["negatives"][s].tolist()
        assert not set(got.tolist()) & set(index.tolist())
        assert torch.randperm(c["num_patches"]).tolist() == g["patch_perms"][s].tolist()       # the generator stands where the reference's second draw found it
        torch.manual_seed(po.step_seed(s))
        assert po.draw_negatives(c["data_size"], index, c["num_negatives"]).tolist() == got.tolist()       # the element-wise filter gives the same
    torch.manual_seed(7)
    few = sample_negatives(10, torch.arange(4), 100)               # fewer rows left than asked for: all of them
    assert sorted(few.tolist()) == list(range(4, 10))


def test_oracle_losses_match_the_reference(golden):
    g = golden["pirl_level"]
    for tag, b, d, k, n, normalize, temperature, weight, seed in po.LOSS_CASES:
        img, patch, bank, pos, neg = po.loss_case_inputs(b, d, k, n, seed)
        assert not set(pos.tolist()) & set(neg.tolist()) and neg.numel() == k
        img.requires_grad_(), patch.requires_grad_()
        loss = po.pirl_loss(img, patch, bank[pos], bank[neg], normalize, temperature, weight)
        loss.backward()
        np.testing.assert_allclose(loss.item(), g[f"loss_{tag}"], rtol=1e-6, err_msg=tag)
        np.testing.assert_allclose(img.grad.numpy(), g[f"loss_{tag}_dimg"], rtol=1e-6, atol=1e-9, err_msg=tag)
        np.testing.assert_allclose(patch.grad.numpy(), g[f"loss_{tag}_dpatch"], rtol=1e-6, atol=1e-9, err_msg=tag)


def test_oracle_bank_matches_the_reference(golden):
    bank = torch.zeros(40, 32)
    for j, (idx, vec) in enumerate(po.bank_case_inputs()):
        po.bank_update(bank, idx, vec, 0.0 if j == 0 else 0.5)
    np.testing.assert_array_equal(bank.numpy(), golden["pirl_level"]["bank_case"])


def test_oracle_trainer_matches_the_reference(golden):
    """Init checksums exact; the bank after the initialisation pass; three seeded steps whose losses stay within 3 x the reference's own fp32-vs-fp64
    distance (floor rtol 1e-5), which the fixture records."""
    g = golden["pirl_level"]
    o = po.PirlOracle(**po.TRAINER)
    state = o.state()
    assert [k for k, v in state.items() if v.dtype.is_floating_point] == [str(k) for k in g["init_keys"]]
    for k, ref in zip(g["init_keys"], g["init_sums"]):
        np.testing.assert_allclose(np.array(oracle.tensor_checksum(state[str(k)].detach().contiguous())), ref, rtol=0, atol=0, err_msg=str(k))
    o.initialize_memory_vectors(po.init_batches())
    np.testing.assert_allclose(o.bank.numpy(), g["bank_init"], rtol=1e-4, atol=1e-5)
    bound = np.maximum(1e-5 * np.abs(g["losses_f64"]), 3 * np.abs(g["losses"] - g["losses_f64"]))
    for s in range(po.STEPS):
        batch = po.step_batch(s)
        torch.manual_seed(po.step_seed(s))
        loss = o.train_step(batch["index"], batch["aug_1"], batch["aug_2"])["loss"]
        assert o.last_negatives.tolist() == g["negatives"][s].tolist() and o.last_permutation.tolist() == g["patch_perms"][s].tolist()
        assert abs(loss - g["losses"][s]) <= bound[s], (s, loss, float(g["losses"][s]), float(bound[s]))


def test_config_has_the_reference_keys():
    cfg = yaml.safe_load(open(os.path.join(ROOT, "self-supervised-vision_amd", "configs", "pirl.yaml")))
    want = {"epochs": 1000, "eval_every": 5, "momentum": 0.5, "proj_dim": 128, "patch_size": 16, "num_patches": 4, "num_negatives": 1000}
    assert {k: cfg[k] for k in want} == want
    assert cfg["encoder"] == {"reduce_bottom_conv": True} and cfg["loss_fn"] == {"normalize": True, "temperature": 0.07, "loss_weight": 0.5}
    assert cfg["optimizer"]["name"] == "sgd" and cfg["optimizer"]["lr"] == 0.01 and cfg["optimizer"]["weight_decay"] == 1e-4
    assert cfg["scheduler"] == {"name": "cosine", "warmup_epochs": 0} and cfg["linear_eval"] == {"epochs": 100, "input_dim": 128, "batch_size": 256, "lr": 0.1}
    assert cfg["data"]["batch_size"] == 256 and cfg["data"]["dataset_name"] == "cifar10"
    assert list(cfg["data"]["transforms"]["train"]) == ["color_jitter", "random_gray", "random_resized_crop", "random_flip", "to_tensor", "normalize"]
    assert cfg["data"]["transforms"]["train"]["random_resized_crop"] == {"size": [32, 32], "scale": [0.6, 1.0]}
    size = cfg["data"]["transforms"]["train"]["random_resized_crop"]["size"]
    assert (size[0] // cfg["patch_size"]) * (size[1] // cfg["patch_size"]) == cfg["num_patches"]


def _forms():
    import test_gpu_pirl_forms as forms
    return forms


def test_case_table_covers_every_documented_branch():
    """Every branch label of the docstring of tests/test_gpu_pirl_forms.py is targeted by a case of the entry point it documents, no case names an unknown label,
    ids are unique, and the bounds respect their caps."""
    import math
    forms = _forms()
    doc = forms.documented_labels()
    assert len(doc) >= 22
    used = {}
    for c in forms.CASES:
        used.update({b: "ssv_pirl_loss_fwd_bwd" for b in c.labels})
    used.update({label: "ssv_bank_momentum_update" for label, _ in forms.BANK_CASES})
    used.update({label: "ssv_patch_split" for label, _ in forms.PATCH_CASES})
    assert not set(doc) - set(used), f"documented branches without a case: {sorted(set(doc) - set(used))}"
    assert not set(used) - set(doc), f"cases name undocumented branches: {sorted(set(used) - set(doc))}"
    assert all(doc[b] == entry for b, entry in used.items())
    ids = [c.id for c in forms.CASES]
    assert len(ids) == len(set(ids))
    assert set(forms.FACTOR) == set(forms.FLOOR) == {"pirl.loss", "pirl.bank"}
    assert all(1.0 <= f <= 8.0 and math.log2(f).is_integer() for f in forms.FACTOR.values()) and all(0.0 <= f <= 16 * 2.0 ** -24 for f in forms.FLOOR.values())


def test_the_accuracy_bounds_are_what_the_committed_report_implies():
    """FACTOR = the worst measured ratio of profiles/kmeans_pirl_forms_report.json rounded up to the next power of two, never above 8; FLOOR as measured under."""
    import json
    from forms_report import next_pow2
    forms = _forms()
    families = json.load(open(os.path.join(ROOT, "profiles", "kmeans_pirl_forms_report.json")))["families"]
    for name in ("pirl.loss", "pirl.bank"):
        worst = max(families[name]["worst_e_ratio"], families[name]["worst_m_ratio"])
        assert worst <= 8.0 and families[name]["FLOOR"] == forms.FLOOR[name] and forms.FACTOR[name] == next_pow2(worst) == families[name]["FACTOR"], name


def test_form_cases_reach_the_splits_and_widths_their_table_claims():
    """The split plan of ssv_pirl_loss_fwd_bwd and the staged row stride of pirl_lse_k restated for the cases that name them."""
    forms = _forms()
    src = open(os.path.join(ROOT, "self-supervised-vision_amd", "csrc", "pirl.hip")).read()
    assert "splits = std::max(1, std::min(std::min(splits, ntile), 64));" in src and "return w < 512 ? w + 4 : w;" in src
    by = {}
    for c in forms.CASES:
        for b in c.labels:
            by.setdefault(b, []).append(c)
    plans = {b: [forms.plan(c.shape[2], c.splits) for c in by[b] if c.splits] for b in ("lse.split_ragged", "lse.split_thin", "lse.split_clamp", "lse.split_max")}
    assert plans["lse.split_ragged"][0] == (10, 3, 4) and plans["lse.split_thin"] == [(10, 1, 10)] and plans["lse.split_clamp"] == [(3, 1, 3)]
    assert plans["lse.split_max"] == [(66, 2, 33)]
    assert all(c.splits == 0 for c in by["lse.split_default"]) and len(by["lse.split_default"]) >= 10
    widths = sorted(c.shape[1] for c in by["lse.width"])
    assert widths == [4, 8, 12, 36, 68, 128, 508, 512]
    lda = lambda d: 8 * ((d + 7) // 8) + (4 if 8 * ((d + 7) // 8) < 512 else 0)
    assert lda(508) == 512 and lda(512) == 512 and lda(128) == 132 and {d % 8 for d in widths} == {0, 4}
    assert sorted(c.shape[2] for c in by["lse.k_edge"]) == [31, 32, 33] and sorted(c.shape[0] for c in by["lse.b_edge"]) == [1, 31, 32]
    assert {c.weight for c in by["lse.weight_edge"]} == {0.0, 1.0}
    assert all(c.normalize == (0,) and c.scale == 6.0 and c.temperature == 0.05 for c in by["lse.online_max"])
    for c in by["lse.online_max"]:                                   # "logits of several hundred"
        _, _, bank, pos, neg = forms.loss_inputs(c)
        assert float((bank[pos] @ bank[neg].t()).abs().max()) / c.temperature > 200.0


@pytest.mark.parametrize("position", range(len(_forms().CASES)), ids=lambda i: _forms().CASES[i].id)
def test_forms_reference_is_well_conditioned(position):
    """ref32 within 1e-3 of ref64 (e and m) and the fp64 loss finite, for every tensor of every loss case (a gradient under a zero weight is identically zero in
    both); the out-of-range indices are where the table says."""
    from forms_report import errors
    forms = _forms()
    case = forms.CASES[position]
    inp = forms.loss_inputs(case)
    b, d, k, n = case.shape
    pos, neg = inp[3], inp[4]
    outside = (neg < 0) | (neg >= n)
    assert int(outside.sum()) == {None: 0, "pos": 0, "neg": 3, "tile": 34}[case.bad] and bool(((pos < 0) | (pos >= n)).any()) == (case.bad == "pos")
    assert len(set(pos.tolist())) == b and neg.numel() == k
    if case.bad == "tile":
        assert bool(outside[32:64].all())
    if case.bad == "pos":
        return
    for normalize in case.normalize:
        r64, r32 = forms.loss_reference(case, inp, torch.float64, normalize), forms.loss_reference(case, inp, torch.float32, normalize)
        assert bool(torch.isfinite(r64["loss"])) and r64["loss"].dtype == torch.float64 and r32["loss"].dtype == torch.float32
        for name, t in r64.items():
            assert bool(torch.isfinite(t).all()) and bool(torch.isfinite(r32[name]).all()), name
            if not float(t.abs().max()) > 0:
                assert case.weight in (0.0, 1.0) and not float(r32[name].abs().max()) > 0
                continue
            e, m = errors(r32[name], t)
            print(f"{case.id} normalize {normalize} {name}: e(ref32) {e:.3e} m(ref32) {m:.3e}")
            assert e <= forms.COND and m <= forms.COND, (name, e, m)


def test_forms_bank_reference_is_well_conditioned():
    from forms_report import errors
    forms = _forms()
    for position, (label, p) in enumerate(forms.BANK_CASES):
        bank, index, z = forms.bank_inputs(position)
        assert len(set(index.tolist())) == p["n"] and int(index.min()) >= 0 and int(index.max()) < p["N"]
        r64, r32 = (forms.bank_reference(bank, index, z, p["m"], dt) for dt in (torch.float64, torch.float32))
        e, m = errors(r32[index], r64[index])
        assert bool(torch.isfinite(r64).all()) and float(r64[index].abs().max()) > 0 and e <= forms.COND and m <= forms.COND, (label, e, m)


def test_masked_reference_is_the_loss_on_the_filtered_index_list():
    """What lse.bad_neg / lse.bad_tile are held to: po.pirl_loss on the negatives that lie inside the bank - spelled out by hand here, and equal to masking the
    out-of-range columns out of both soft-max denominators."""
    forms = _forms()
    for case in (c for c in forms.CASES if c.bad in ("neg", "tile")):
        img, patch, bank, pos, neg = forms.loss_inputs(case)
        n = bank.shape[0]
        kept = [int(i) for i in neg.tolist() if 0 <= i < n]
        assert len(kept) == (67 if case.bad == "neg" else 36)
        for normalize in case.normalize:
            got = forms.loss_reference(case, (img, patch, bank, pos, neg), torch.float64, normalize)
            zi, zp = img.double().requires_grad_(), patch.double().requires_grad_()
            rows = bank.double()
            temperature, weight = 1.0 / forms._s(1.0 / case.temperature), forms._s(case.weight)
            by_hand = po.pirl_loss(zi, zp, rows[pos], rows[torch.tensor(kept)], bool(normalize), temperature, weight)
            by_hand.backward()
            assert got["loss"].item() == by_hand.item() and torch.equal(got["d_img"], zi.grad) and torch.equal(got["d_patch"], zp.grad)
            # the same with every column present and the out-of-range ones at -inf
            vi, vp = (torch.nn.functional.normalize(t, dim=-1) if normalize else t for t in (img.double(), patch.double()))
            m = rows[pos]
            inside = (neg >= 0) & (neg < n)
            logits = (m @ rows[neg.clamp(0, n - 1)].t() / temperature).masked_fill(~inside[None, :], float("-inf"))
            terms = [torch.logsumexp(torch.cat((p, logits), 1), 1) - p[:, 0] for p in ((m * vp).sum(1, keepdim=True) / temperature, (m * vi).sum(1, keepdim=True) / temperature)]
            masked = (weight * terms[0] + (1.0 - weight) * terms[1]).mean()
            assert abs(masked.item() - by_hand.item()) <= 1e-12 * abs(by_hand.item())


def test_pirl_loss_needs_the_gpu():
    from ssv_amd import _lib
    from ssv_amd.utils import losses
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    img, patch, bank, pos, neg = po.loss_case_inputs(4, 8, 6, 16, 1)
    with pytest.raises(_lib.SsvError):
        losses.PirlLoss()(img, patch, bank, pos, neg)
