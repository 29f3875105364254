"""CPU: the host side of the DenseCL trainer (models/densecl.py, csrc/densecl.hip) - the oracle against cases worked by hand, the command line, the configs, the
ABI surface, the workspace sizing and its plan, and the conditions the kernel tests' case tables must meet so that their fp32 reference means something."""
import ctypes as C
import json
import math
import os
import re

import pytest
import torch
import yaml

import densecl_oracle as do

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "self-supervised-vision_amd", "configs")
HEADER = os.path.join(ROOT, "include", "ssv_hip.h")
ARITHS = ("bf16x3", "f32")


def test_oracle_agrees_with_a_hand_worked_two_key_case():
    """q = (1, 0), positive (1, 0), one bank row (0, 1), inv_temp 2: s+ = 2, s_0 = 0, lse = log(e^2 + 1), p+ = e^2 / (e^2 + 1),
    dq = 2 (p+ k+ + p_0 b_0 - k+) = (2 (p+ - 1), 2 p_0)"""
    q = torch.tensor([[1.0, 0.0]])
    keys = torch.tensor([[0.0, 1.0], [1.0, 0.0]])
    bank = torch.tensor([[0.0, 1.0], [5.0, 5.0]])                         # the row behind K = 1 is not read
    out = do.queue_nce(q, keys, torch.tensor([1], dtype=torch.int32), bank, 1, 2.0)
    lse = math.log(math.exp(2.0) + 1.0)
    pp, p0 = math.exp(2.0 - lse), math.exp(-lse)
    assert abs(float(out["lse"][0]) - lse) < 1e-14 and abs(float(out["loss"]) - (lse - 2.0)) < 1e-14
    assert torch.allclose(out["dq"], torch.tensor([[2.0 * (pp - 1.0), 2.0 * p0]], dtype=torch.float64), atol=1e-14, rtol=0)
    assert abs(out["pos"] - pp) < 1e-14 and out["smax"] == 2.0
    assert do.queue_nce(q, keys, torch.tensor([1], dtype=torch.int32), bank, 1, 2.0, torch.float32)["dq"].dtype == torch.float32
    # a zero bank row scores 0 and counts: lse = log(e^2 + 1) again, whatever the row's direction would have been
    zero = do.queue_nce(q, keys, torch.tensor([1], dtype=torch.int32), torch.zeros(1, 2), 1, 2.0)
    assert abs(float(zero["lse"][0]) - lse) < 1e-14
    # the trainer's loss is the convex combination of MoCo's and the dense term
    both = do.densecl_loss(q, keys[1:], bank, 1, q, keys, torch.tensor([1], dtype=torch.int32), bank, 1, 0.5, 0.25)
    assert abs(float(both["global"]) - (lse - 2.0)) < 1e-14 and abs(float(both["loss"]) - (0.75 * float(both["global"]) + 0.25 * float(both["dense"]))) < 1e-15


def test_match_oracle_on_a_hand_worked_case():
    """one image, two cells: f1 = ((1, 0), (0, 0)), f2 = ((3, 4), (2, 0)): cell 0 scores (3 / 5, 2 / 2) and picks 1 with cosine 1; the zero row picks 0"""
    f1 = torch.tensor([[[1.0, 0.0], [0.0, 0.0]]])
    f2 = torch.tensor([[[3.0, 4.0], [2.0, 0.0]]])
    out = do.dense_match(f1, f2)
    assert out["j"].tolist() == [[1, 0]] and out["idx"].tolist() == [[1, 0]] and out["sim"].tolist() == [[1.0, 0.0]]
    two = do.dense_match(torch.cat([f1, f1]), torch.cat([f2, f2]))
    assert two["idx"].tolist() == [[1, 0], [3, 2]]                         # rows of the [b * s, d] key grid
    tie = do.dense_match(torch.tensor([[[1.0, 1.0]]]).repeat(1, 3, 1), torch.tensor([[[0.0, 1.0], [2.0, 2.0], [1.0, 1.0]]]))
    assert tie["j"].tolist() == [[1, 1, 1]]                                # cells 1 and 2 tie: the lowest wins


def test_cli_resolves_densecl_and_still_refuses_the_unbuilt():
    from ssv_amd import main as cli
    from ssv_amd.models.base import TwoViewTrainer
    from ssv_amd.models.moco import MoCo
    cls = cli.trainer_class("densecl")
    assert cls.__name__ == "DenseCL" and issubclass(cls, TwoViewTrainer) and issubclass(cls, MoCo)
    assert cls.algo == "densecl" and cls.graph_safe is True and cls.graph_inputs == ("aug_1", "aug_2")
    assert cli.ALGORITHMS["densecl"] == ("densecl", "DenseCL")
    for name in ("deep_cluster", "swav", "sela"):
        assert cli.ALGORITHMS[name] is None
        with pytest.raises(NotImplementedError):
            cli.trainer_class(name)
    assert cli.parse(["-c", "x.yaml", "-a", "densecl", "-m", "resnet18", "-t", "train"])["algo"] == "densecl"


@pytest.mark.parametrize("fname", ["densecl.yaml", "densecl_r18_32_synthetic.yaml"])
def test_configs_parse(fname):
    from ssv_amd import _lib, ops
    from ssv_amd.utils import augmentations, losses
    cfg = yaml.safe_load(open(os.path.join(CONFIGS, fname)))
    block = cfg["densecl"]
    assert sorted(block) == ["dense_queue_size", "loss_lambda"] and block["loss_lambda"] == 0.5 and block["dense_queue_size"] == cfg["queue_size"]
    assert cfg["proj_dim"] == 128 and cfg["proj_dim"] % 32 == 0 and cfg["proj_dim"] <= _lib.QUEUE_NCE_FUSED_MAX_D          # the shipped width takes the fused kernel
    assert ops.queue_nce_route(cfg["proj_dim"]) == ("fused" if ops.ARITHMETIC == "bf16x3" else "unfused")
    assert cfg["loss_fn"] == {"normalize": True, "temperature": 0.2} and cfg["encoder"] == {"reduce_bottom_conv": True}
    moco = yaml.safe_load(open(os.path.join(CONFIGS, "moco.yaml")))
    assert cfg["data"]["transforms"] == moco["data"]["transforms"] and cfg["optimizer"] == moco["optimizer"] and cfg["encoder"] == moco["encoder"]
    assert ("synthetic" in cfg["data"]) == ("synthetic" in fname)
    if "synthetic" in cfg["data"]:
        assert cfg["data"]["batch_size"] == 512
    for split in ("train", "test"):
        assert augmentations.get_transform(cfg["data"]["transforms"][split]) is not None
    fn = losses.DenseNceLoss(**cfg["loss_fn"])
    assert fn.temperature == 0.2 and fn.normalize is True and fn.last_flag is None and fn.last_lse is None


def test_entry_points_are_declared_and_bound():
    from ssv_amd import _lib
    hdr = open(HEADER).read()
    vp, i32, i64, f32, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_size_t
    want = {"ssv_dense_match": (C.c_int, [i32, i32, i32, vp, vp, f32, vp, vp, i32, vp]),
            "ssv_queue_nce_workspace_bytes": (sz, [i32, i64, i32, i32]),
            "ssv_queue_nce": (C.c_int, [i32, i32, i64, i64, vp, vp, vp, vp, f32, vp, vp, vp, vp, i32, vp, sz, vp])}
    for name, sig in want.items():
        assert re.search(rf"^(size_t|int) {name}\(", hdr, re.M), f"{name} is not declared in include/ssv_hip.h"
        assert _lib.SIGNATURES[name] == sig
        assert hasattr(_lib.load(), name)
    for macro, value in (("SSV_DENSE_MATCH_MAX_S", _lib.DENSE_MATCH_MAX_S), ("SSV_DENSE_MATCH_MAX_C", _lib.DENSE_MATCH_MAX_C), ("SSV_QUEUE_NCE_MAX_M", _lib.QUEUE_NCE_MAX_M),
                         ("SSV_QUEUE_NCE_FUSED_MAX_D", _lib.QUEUE_NCE_FUSED_MAX_D), ("SSV_QUEUE_NCE_SLICE", _lib.QUEUE_NCE_SLICE),
                         ("SSV_QUEUE_NCE_MAX_SLICES", _lib.QUEUE_NCE_MAX_SLICES), ("SSV_QUEUE_NCE_TARGET_WGS", _lib.QUEUE_NCE_TARGET_WGS)):
        assert re.search(rf"^#define {macro} {value}$", hdr, re.M), macro
    assert (_lib.DENSE_MATCH_MAX_S, _lib.QUEUE_NCE_MAX_M) == (256, 131072) == (do.MATCH_MAX_S, do.MAX_M)
    assert (_lib.QUEUE_NCE_FUSED_MAX_D, _lib.QUEUE_NCE_SLICE, _lib.QUEUE_NCE_MAX_SLICES, _lib.QUEUE_NCE_TARGET_WGS) == (do.FUSED_MAX_D, do.SLICE, do.MAX_SLICES, do.TARGET_WGS)
    assert _lib.ABI_VERSION == 124 and _lib.load().ssv_version() == 124
    assert "Not built: the data-parallel form, the gradient to keys" in hdr and hdr.count("The ABI version stays 124: entry points were only added.") >= 4
    src = open(os.path.join(ROOT, "self-supervised-vision_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bdensecl\.hip\b", src, re.M)


REFUSED_NCE = [(0, 100, 128), (131073, 100, 128), (16, 0, 128), (16, 1 << 31, 128), (16, 100, 126), (16, 100, 0), (16, 100, 8196), (-3, 100, 128), (16, -1, 128)]      # (m, K, d)


def test_workspace_sizing_and_null_refusals():
    from ssv_amd import _lib
    lib = _lib.load()
    lib.ssv_last_error.restype = C.c_char_p
    for arith in (_lib.ARITH_BF16X3, _lib.ARITH_F32_MFMA):
        for shape in REFUSED_NCE:
            assert lib.ssv_queue_nce_workspace_bytes(*shape, arith) == 0, shape
        assert lib.ssv_queue_nce_workspace_bytes(8192, 4096, 128, arith) > 0 and lib.ssv_queue_nce_workspace_bytes(1, 1, 4, arith) > 0
        assert lib.ssv_queue_nce_workspace_bytes(131072, (1 << 31) - 16, 8192, arith) > 0
    assert lib.ssv_queue_nce_workspace_bytes(131072, (1 << 31) - 1, 128, _lib.ARITH_BF16X3) > 0          # the fused route streams the queue: no padded copy
    assert lib.ssv_queue_nce_workspace_bytes(16, (1 << 31) - 1, 128, _lib.ARITH_F32_MFMA) == 0           # the GEMM route describes it with 32-bit sizes
    assert lib.ssv_queue_nce_workspace_bytes(512, 1750, 128, 5) == 0                                      # no such arithmetic
    assert lib.ssv_queue_nce_workspace_bytes(64, 4096, 36, _lib.ARITH_BF16X3) == lib.ssv_queue_nce_workspace_bytes(64, 4096, 36, _lib.ARITH_F32_MFMA)
    assert lib.ssv_queue_nce(16, 128, 100, 16, None, None, None, None, 5.0, None, None, None, None, _lib.ARITH_BF16X3, None, 0, None) == -1
    assert lib.ssv_last_error().decode().startswith("ssv_queue_nce:")
    assert lib.ssv_queue_nce(16, 128, 100, 0, None, None, None, None, 5.0, None, None, None, None, _lib.ARITH_BF16X3, None, 0, None) == -1
    assert lib.ssv_last_error().decode().startswith("ssv_queue_nce:")
    for shape in ((0, 16, 64), (2, 0, 64), (2, 257, 64), (2, 16, 62), (2, 16, 0), (2, 16, 8196), (1 << 23, 256, 64), (2, 16, 64)):      # the last: a good shape, NULL pointers
        assert lib.ssv_dense_match(*shape, None, None, 1e-12, None, None, _lib.ARITH_BF16X3, None) == -1, shape
        assert lib.ssv_last_error().decode().startswith("ssv_dense_match:")


def test_the_imagenet_workspace_fits_and_grows_no_faster_than_m():
    """The design condition of the plan: 25,088 queries against 65,536 rows of width 128 need at most 512 MiB (the logits would be 6.1 GiB); and the workspace per padded
    query never grows with m - fewer slices as the query tiles fill the machine, then a constant."""
    from ssv_amd import _lib
    lib = _lib.load()
    got = lib.ssv_queue_nce_workspace_bytes(25088, 65536, 128, _lib.ARITH_BF16X3)
    assert 0 < got <= 512 << 20 and got == do.plan(25088, 65536, 128, "bf16x3")["bytes"]
    assert do.plan(25088, 65536, 128, "bf16x3")["slices"] == 1 and do.plan(8192, 4096, 128, "bf16x3")["slices"] == 1
    for d, K in ((128, 65536), (64, 65536), (128, 4096), (32, 513)):
        per = [lib.ssv_queue_nce_workspace_bytes(m, K, d, _lib.ARITH_BF16X3) / ((m + 31) // 32 * 32) for m in (32, 64, 256, 1024, 4096, 8192, 16384, 32768, 65536, 131072)]
        assert all(b <= a * (1 + 1e-9) + 256 for a, b in zip(per, per[1:])), (d, K, per)
    assert lib.ssv_queue_nce_workspace_bytes(131072, 65536, 128, _lib.ARITH_BF16X3) <= 512 << 20


def test_ops_and_loss_refuse_host_tensors_and_bad_shapes():
    from ssv_amd import _lib, ops
    from ssv_amd.utils import losses
    q, k, pos, bank = torch.zeros(4, 8), torch.zeros(6, 8), torch.zeros(4, dtype=torch.int32), torch.zeros(16, 8)
    with pytest.raises(_lib.SsvError):
        ops.queue_nce(q, k, pos, bank, 16, 5.0)                             # CPU tensors: no fallback
    with pytest.raises(_lib.SsvError):
        ops.dense_match(torch.zeros(2, 4, 4, 8), torch.zeros(2, 4, 4, 8))
    fn = losses.DenseNceLoss(True, 0.2)
    bad = ((torch.zeros(4, 6), torch.zeros(6, 6), pos, torch.zeros(16, 6)),          # D % 4
           (q, torch.zeros(6, 12), pos, bank), (q, k, pos, torch.zeros(16, 12)),    # widths differ
           (torch.zeros(8), k, pos, bank), (q, k, torch.zeros(5, dtype=torch.int32), bank), (q, k, torch.zeros(4, 1, dtype=torch.int32), bank),
           (torch.zeros(_lib.QUEUE_NCE_MAX_M + 1, 8), k, torch.zeros(_lib.QUEUE_NCE_MAX_M + 1, dtype=torch.int32), bank))
    for args in bad:
        with pytest.raises(ValueError):
            fn(*args)
    with pytest.raises(ValueError):
        losses.DenseNceLoss(True, 0.0)(q, k, pos, bank)
    assert ops.queue_nce_route(128) == ("fused" if ops.ARITHMETIC == "bf16x3" else "unfused")
    assert ops.queue_nce_route(36) == "unfused" and ops.queue_nce_route(160) == "unfused"
    with ops.arithmetic("f32"):
        assert ops.queue_nce_route(128) == "unfused"
    ops.check_queue_nce_flag(None)
    ops.check_queue_nce_flag(torch.zeros(1, dtype=torch.int32))
    with pytest.raises(_lib.SsvError):
        ops.check_queue_nce_flag(torch.ones(1, dtype=torch.int32))


def test_loss_module_is_single_process(monkeypatch):
    from ssv_amd import distributed as hdist
    from ssv_amd.utils import losses
    monkeypatch.setattr(hdist, "is_on", lambda: True)
    with pytest.raises(NotImplementedError):
        losses.DenseNceLoss()(torch.zeros(4, 8), torch.zeros(6, 8), torch.zeros(4, dtype=torch.int32), torch.zeros(16, 8))


def test_the_encoder_keeps_its_pooling_behind_the_feature_map():
    """ResNet._run is the pooling of ResNet._feature_map - the split DenseCL's module relies on - and DenseCL's module builds encoder, proj_head, dense_head in
    that order, so the first two draw MoCo's weights at the same seed"""
    import inspect
    from ssv_amd.models import densecl, moco
    from ssv_amd.networks import resnet
    assert "hnn.global_avgpool(tape, self._feature_map(tape, x))" in inspect.getsource(resnet.ResNet._run)
    torch.manual_seed(3)
    a = moco.EncoderModel(resnet.resnet18(reduce_bottom_conv=True), 512, 128)
    torch.manual_seed(3)
    b = densecl.DenseEncoderModel(resnet.resnet18(reduce_bottom_conv=True), 512, 128)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sb)[:len(sa)] == list(sa) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert [k for k in sb if k not in sa] == [f"dense_head.{n}" for n in ("layer1.0.weight", "layer1.0.bias", "layer1.1.weight", "layer1.1.bias", "layer1.1.running_mean",
                                                                           "layer1.1.running_var", "layer1.1.num_batches_tracked", "layer2.weight", "layer2.bias")]
    assert sb["dense_head.layer1.0.weight"].shape == (512, 512) and sb["dense_head.layer2.weight"].shape == (128, 512)


# ---- the case tables ----------------------------------------------------------------------------------------------------------------------------------------------
def test_case_table_covers_the_mechanisms():
    cases = do.cases()
    assert len(set(cases)) == len(cases)
    assert {c[0] for c in cases} >= {1, 33, 70} and {c[1] for c in cases} == {32, 64, 96, 128, 4, 36, 160} and {c[2] for c in cases} == {1, 31, 33, 513, 640}
    assert {c[3] for c in cases} == set(do.VARIANTS) == {"plain", "same", "late", "dup", "zero"}
    assert all(k % 16 for k in (1, 31, 33, 513)) and 640 % 16 == 0 and 2 * do.SLICE < 513 <= 2 * do.SLICE + 32 and 640 > 2 * do.SLICE
    for case in cases:
        q, keys, pos, bank, K, it = do.make_case(case)
        m, d, k, variant = case
        assert q.shape == (m, d) and keys.shape == (m + 3, d) and pos.shape == (m,) and pos.dtype == torch.int32 and bank.shape == (k, d) and K == k and it == 5.0
        assert 0 <= int(pos.min()) and int(pos.max()) < m + 3
        if variant == "same":
            assert len(set(pos.tolist())) == 1
        elif m >= 33:
            assert 0 in pos.tolist() and m + 2 in pos.tolist()
        if variant == "dup":
            assert torch.equal(bank[255], bank[256]) and do.plan(m, k, d, "bf16x3").get("rows", do.SLICE) == do.SLICE
        if variant == "zero":
            assert float(bank.abs().max()) == 0.0


@pytest.mark.parametrize("case", do.cases(), ids=do.case_id)
def test_case_table_keeps_the_fp32_reference_meaningful(case):
    """In fp64: the mean probability of the positive is below 0.9 (dq is no cancellation), no score leaves [-60, 60] and dq is not all zero"""
    q, keys, pos, bank, K, it = do.make_case(case)
    ref = do.queue_nce(q, keys, pos, bank, K, it)
    assert ref["pos"] < 0.9, ref["pos"]
    assert ref["smax"] <= 60.0, ref["smax"]
    assert float(ref["dq"].abs().max()) > 0.0 and float(ref["loss"]) > 0.0
    if case[3] == "late":                                                  # the largest score of every query is the last bank row's (and above the positive's)
        sc = q.double() @ bank.double().T
        assert bool((sc.argmax(dim=1) == K - 1).all())


@pytest.mark.parametrize("seed", do.MATCH_SEEDS)
@pytest.mark.parametrize("case", do.MATCH_CASES, ids=do.match_id)
def test_match_cases_keep_the_fp32_reference_meaningful(case, seed):
    """The fp32 evaluation of the oracle picks the fp64 arg-max in every cell, and the smallest fp64 gap between the best and the second-best cosine is at least
    1e-6 (a planted copy counts as its original), so the kernel test's reference needs no excuse itself"""
    f1, f2 = do.make_match_case(case, seed)
    b, s, c, variant = case
    assert f1.shape == f2.shape == (b, s, c) and float(f1.min()) >= 0.0
    r64, r32 = do.dense_match(f1, f2), do.dense_match(f1, f2, dtype=torch.float32)
    gap = do.match_gap(case, r64)
    print(f"{do.match_id(case)} seed {seed}: smallest gap {gap:.3g}")
    assert torch.equal(r64["j"], r32["j"]) and gap >= 1e-6
    if variant == "planted":
        assert torch.equal(f2[0, 7], f2[0, 3]) and int(r64["j"][0, 0]) == 3 and not bool((r64["j"][0] == 7).any())
        assert int(r64["j"][b - 1, 1]) == 0 and float(r64["sim"][b - 1, 1]) == 0.0 and not bool((r64["j"][b - 1][torch.arange(s) != 1] == 2).any())
    assert {cs[:3] for cs in do.MATCH_CASES} == {(3, 1, 8), (5, 16, 64), (4, 49, 512), (3, 50, 36), (2, 256, 128), (1, 256, 2048)}


# ---- the launch forms ---------------------------------------------------------------------------------------------------------------------------------------------
def test_plan_restatement_is_the_librarys():
    """densecl_oracle.plan against what the library exposes of its plan - the workspace size in both arithmetics - at every case and at shapes around each
    threshold; and the dispatch lines it restates"""
    from ssv_amd import _lib
    src, hdr = (open(os.path.join(ROOT, "self-supervised-vision_amd", "csrc", f)).read() for f in ("densecl.hip", "bank_softmax.h"))
    # the tile rule, the chunk rule and the <DT, KT> ladder are written once, in the header; the file names them
    assert "p.KT = (p.T == 1 || p.DT >= 3) ? 1 : 2;" in hdr and f"constexpr int CHUNK_ROWS = {do.CHUNK_ROWS};" in hdr and "CHUNK_ELEMS = 1ll << 25;" in hdr
    assert "if ((p).DT == 4) hipLaunchKernelGGL((KERNEL<4, 1>)" in hdr and "else if ((p).DT == 3) hipLaunchKernelGGL((KERNEL<3, 1>)" in hdr
    assert "banksm::plan_tiles(p, m, d);" in src and "p.cr = banksm::chunk_rows(p.kp, m);" in src and "SSV_FUSED_LADDER(qn_fused_k, p," in src
    assert "int64_t want = cdiv(TARGET_WGS, blocks);" in src
    assert "hipGetDeviceProperties" not in src and "ssv_device_cus" not in src            # the plan never asks the device for its size
    lib = _lib.load()
    shapes = [(c[0], c[2], c[1]) for c in do.cases()]
    shapes += [(m, K, d) for m in (1, 32, 33, 64, 65, 1024, 1025, 2720, 2721, 2752, 4064, 4065, 4096, 4097, 8160, 8161, 8192, 8193, 16320, 16321, 16352, 16353, 25088, 131072)
               for d in (32, 64, 96, 128, 132, 160, 4) for K in (1, 255, 256, 257, 640, 4096, 65536)]
    shapes += [(40, K, 32) for K in (do.SLICE * do.MAX_SLICES, do.SLICE * do.MAX_SLICES + 1, 1 << 20)] + [(2000, 40000, 36), (5, (1 << 25) + 1, 36)]
    for m, K, d in shapes:
        for arith in ARITHS:
            code = _lib.ARITH_BF16X3 if arith == "bf16x3" else _lib.ARITH_F32_MFMA
            p = do.plan(m, K, d, arith)
            assert lib.ssv_queue_nce_workspace_bytes(m, K, d, code) == p["bytes"], (m, K, d, arith)
            assert p["fused"] == (arith == "bf16x3" and d % 32 == 0 and d <= do.FUSED_MAX_D)
            if p["fused"]:
                assert p["rows"] % do.SLICE == 0 and 1 <= p["slices"] <= do.MAX_SLICES and p["slices"] * p["rows"] >= K > (p["slices"] - 1) * p["rows"]
                assert p["slices"] == 1 or (p["slices"] - 1) * p["blocks"] < do.TARGET_WGS      # slices only as far as a small m needs them


def test_cases_reach_every_launch_form():
    """All six (DT, KT) instantiations the dispatch of ssv_queue_nce can launch; the sliced and the unsliced plan (three, two and one slice at K = 640, each
    reached by an m just past its threshold); many slices of more than SSV_QUEUE_NCE_SLICE rows need K > 8192 and run in tests/test_gpu_dense_nce_forms.py (FORM_CASES, below); more than one chunk
    of the unfused route in both arithmetics; the unfused route under bf16x3 at a width that is a multiple of 32; both tile counts of the matching kernel"""
    plans = {c: do.plan(c[0], c[2], c[1], "bf16x3") for c in do.cases()}
    assert {(p["DT"], p["KT"]) for p in plans.values() if p["fused"]} == {(1, 1), (1, 2), (2, 1), (2, 2), (3, 1), (4, 1)}
    assert {p["slices"] for c, p in plans.items() if p["fused"] and c[2] == 640} == {1, 2, 3}
    for (m, d, K, v), want in (((4129, 128, 640, "plain"), 2), ((8225, 128, 640, "plain"), 1), ((8225, 64, 640, "plain"), 2), ((16417, 64, 640, "plain"), 1)):
        assert plans[(m, d, K, v)]["slices"] == want
        assert do.plan(m - 128, K, d, "bf16x3")["slices"] == want + 1, "the case no longer sits within four query tiles of its threshold"
    assert all(p["slices"] == 1 for c, p in plans.items() if p["fused"] and c[2] <= do.SLICE)
    for arith in ARITHS:
        assert max(do.plan(c[0], c[2], c[1], arith).get("chunks", 1) for c in do.cases()) >= 9
        assert any(not do.plan(c[0], c[2], c[1], arith)["fused"] and c[1] == 160 and c[0] > do.CHUNK_ROWS for c in do.cases())
    assert any(not p["fused"] and c[1] % 32 == 0 for c, p in plans.items())
    assert {s <= 128 for _, s, _, _ in do.MATCH_CASES} == {True, False}
    assert set(do.ROUTES_AGREE) <= set(do.cases()) and all(plans[c]["fused"] for c in do.ROUTES_AGREE)


def test_the_accuracy_bound_is_what_the_committed_report_implies():
    """FACTOR of tests/test_gpu_dense_nce.py = the worst measured ratio of profiles/dense_nce_kernels_report.json rounded up to the next power of two, never above
    8; every case and both arithmetics are in the report"""
    doc = json.load(open(os.path.join(ROOT, "profiles", "dense_nce_kernels_report.json")))
    worst = max(max(v["ratio_e"], v["ratio_m"]) for v in doc["cases"].values())
    assert worst == doc["worst_ratio"] <= 8.0 and doc["floor"] == do.FLOOR and do.FACTOR == do.next_pow2(worst) == doc["factor"]
    want = {f"{do.case_id(c)}[{a}].{k}" for c in do.cases() for a in ARITHS for k in ("loss", "lse", "dq")}
    want |= {f"match-{do.match_id(c)}[{a}].sim" for c in do.MATCH_CASES for a in ARITHS}
    assert set(doc["cases"]) == want and re.fullmatch(r"[0-9a-f]{16}", doc["source_sha16"])


# ---- the launch forms of tests/test_gpu_dense_nce_forms.py and tests/test_gpu_dense_match_forms.py ----------------------------------------------------------------
def test_form_cases_reach_every_launch_form():
    """Every case of densecl_oracle.FORM_CASES reaches, by the restated plan (held against the library's workspace size here too), the form its label names in
    each arithmetic; between them the labels see what the older table leaves out: a slice of 2 * SLICE rows in four instantiations with a last slice of 8 rows,
    K on either side of one slice and one row into every quarter, the clamped chunk of the unfused route in both arithmetics, the largest m; and the label
    table of the GPU file is the one its cases name."""
    import test_gpu_dense_nce_forms as forms
    from ssv_amd import _lib
    lib = _lib.load()
    cases = do.FORM_CASES
    assert len(set(cases)) == len(cases) == 18 and not set(cases) & set(do.cases()) and set(do.FORM_ROUTES_AGREE) <= set(cases) and len(do.FORM_ROUTES_AGREE) == 2
    assert {c[3] for c in do.FORM_ROUTES_AGREE} == {"late", "climb"} and all(c[2] == do.LONG for c in do.FORM_ROUTES_AGREE)
    assert set(forms.CASE_LABELS) == set(cases) and forms.ARITHS == ARITHS
    for case, labels in forms.CASE_LABELS.items():
        m, d, K, _ = case
        for arith, label in zip(ARITHS, labels):
            assert not label or forms.reaches(label, case, arith), (case, arith, label)
            assert not forms.reaches("quarter.edge" if label != "quarter.edge" else "m.max", case, arith)       # reaches() tells the forms apart
            code = _lib.ARITH_BF16X3 if arith == "bf16x3" else _lib.ARITH_F32_MFMA
            assert lib.ssv_queue_nce_workspace_bytes(m, K, d, code) == do.plan(m, K, d, arith)["bytes"] <= 160 << 20, (case, arith)
    by = lambda label, a: [c for c, l in forms.CASE_LABELS.items() if l[a] == label]
    plans = lambda label, arith: [do.plan(c[0], c[2], c[1], arith) for c in by(label, ARITHS.index(arith))]
    # slice.long: L = 512, 17 slices, the last of 8 rows (three empty quarters, quarter 0 clipped at K); four instantiations; unfused at d = 36 and under f32
    long_ = plans("slice.long", "bf16x3")
    assert {(p["DT"], p["KT"]) for p in long_ if p["fused"]} == {(1, 2), (4, 1), (2, 1), (2, 2)} and sum(not p["fused"] for p in long_) == 1
    assert all((p["rows"], p["slices"]) == (2 * do.SLICE, 17) and do.LONG - 16 * p["rows"] == 8 for p in long_ if p["fused"])
    assert all(p["kp"] == 8208 for p in plans("slice.long", "f32")) and all(p.get("rows", 0) <= do.SLICE or p["slices"] <= 2 for p in (do.plan(c[0], c[2], c[1], "bf16x3") for c in do.cases()))      # the older table: one or two long slices at most
    assert {c[3] for c in by("slice.long", 0)} == {"plain", "late", "dupL"} and do.FORM_DUP_ROW == 2 * do.SLICE
    assert {c[2] for c in by("slice.edge", 0)} == {do.SLICE - 1, do.SLICE, do.SLICE + 1} and {p["kp"] for p in plans("slice.edge", "f32")} == {256, 272}
    assert {c[2] for c in by("quarter.edge", 0)} == {65, 129, 193} and {p["DT"] for p in plans("quarter.edge", "bf16x3")} == {1, 3, 4}
    for arith in ARITHS:
        clamp = plans("chunk.clamp", arith)
        assert len(clamp) == 2 and all((p["cr"], p["chunks"], p["kp"]) == (1023, 2, 32800) for p in clamp) and {c[1] for c in by("chunk.clamp", 0)} == {4, 36}
        assert all(do.plan(c[0], c[2], c[1], arith).get("cr", 0) != 1023 for c in do.cases())
    assert {(c[1], c[2]) for c in by("temp.climb", 0)} == {(96, 640), (64, do.LONG), (128, do.LONG), (36, 640)}
    assert [(p["T"], p["blocks"]) for p in plans("m.max", "bf16x3")] == [(4096, 2048)] and [p["chunks"] for p in plans("m.max", "f32")] == [128]
    assert max(c[0] for c in do.cases()) < do.MAX_M == by("m.max", 0)[0][0]
    doc = forms.documented_labels()
    assert len(doc) == 9 and set(doc.values()) == {"ssv_queue_nce"}
    used = {b for labels in forms.TARGETS.values() for b in labels.split()}
    assert not set(doc) - used, f"documented branches without a case: {sorted(set(doc) - used)}"
    assert not used - set(doc), f"cases name undocumented branches: {sorted(used - set(doc))}"
    assert set(forms.TARGETS) == {name for name in dir(forms) if name.startswith("test_")}


@pytest.mark.parametrize("case", do.FORM_CASES, ids=do.case_id)
def test_form_cases_keep_the_fp32_reference_meaningful(case):
    """In fp64: the mean probability of the positive is below 0.9, no score leaves [-60, 60] and dq is not zero; the planted variants are what they say"""
    q, keys, pos, bank, K, it = do.make_case(case)
    m, d, k, variant = case
    assert q.shape == (m, d) and keys.shape == (m + 3, d) and pos.shape == (m,) and pos.dtype == torch.int32 and bank.shape == (k, d) and K == k
    assert 0 <= int(pos.min()) and int(pos.max()) < m + 3 and it == (do.CLIMB_INV_TEMP if variant == "climb" else 5.0)
    ref, r32 = do.queue_nce(q, keys, pos, bank, K, it), do.queue_nce(q, keys, pos, bank, K, it, dtype=torch.float32)
    print(f"{do.case_id(case)}: pos {ref['pos']:.3g} smax {ref['smax']:.3g} e(ref32) of dq {do.errs(r32['dq'], ref['dq'])[0]:.3g}")
    assert ref["pos"] < 0.9, ref["pos"]
    assert ref["smax"] <= 60.0, ref["smax"]
    assert float(ref["dq"].abs().max()) > 0.0 and float(ref["loss"]) > 0.0
    if variant == "late":
        assert bool(((q.double() @ bank.double().T).argmax(dim=1) == K - 1).all())
    if variant == "dupL":
        r = do.FORM_DUP_ROW
        assert torch.equal(bank[r], bank[r - 1]) and do.plan(m, k, d, "bf16x3")["rows"] == r and not torch.equal(bank[r], bank[r + 1])
    if variant == "climb":
        assert abs(it - 1.0 / 0.07) < 1e-12
        raised, tiles = do.climbing_tiles(q, bank)
        print(f"{do.case_id(case)}: {raised:.1f} of {tiles} tiles raise the running maximum")
        if k == 640:
            assert tiles == 20 and raised >= 0.25 * tiles, raised
        assert raised >= 5.0, raised


def test_match_form_cases_reach_their_labels():
    """Every case of densecl_oracle.FORM_MATCH_CASES is the form its label names, and the labels between them hold every edge of dm_match_k's tiling: s on both
    sides of each tile of NT = 1, the NT switch, an empty second tile, the clamp inside the last tile, every accumulator position, the slab tails and both
    channel limits"""
    import test_gpu_dense_match_forms as forms
    cases = do.FORM_MATCH_CASES
    assert len(set(cases)) == len(cases) == 22 and not set(cases) & set(do.MATCH_CASES) and set(forms.CASE_LABELS) == set(cases) and forms.ARITHS == ARITHS
    for case, label in forms.CASE_LABELS.items():
        assert forms.reaches(label, case), (case, label)
        if label != "c.edge":                                              # reaches() tells the forms apart (the channel edges run at map sizes of their own)
            assert not any(forms.reaches(other, case) for other in ("tile.edge", "nt.switch", "rows.all", "ties.cross", "eps.clamp", "nan.cell", "c.edge") if other != label), case
    by = lambda label: [c for c, l in forms.CASE_LABELS.items() if l == label]
    assert {c[1] for c in by("tile.edge")} == {32, 33, 64, 65, 96, 97} and any(c[0] % -(-c[1] // 32) for c in by("tile.edge"))
    assert {c[1] for c in by("nt.switch")} == {128, 129, 160, 255}
    assert {c[1] for c in by("rows.all")} == {256, 129, 33} and {c[2] for c in by("c.edge")} == {4, 12, 24, 8, do.MATCH_MAX_C}
    assert all(c[3] == ("plain" if c[2] == do.MATCH_MAX_C else "signed") for c in by("c.edge"))
    # a permutation of 256 cells wins at every (wave, t, half, r) exactly once
    assert len({forms.position(j) for j in range(256)}) == 256 == 4 * 2 * 2 * 16
    assert [forms.position(j)[:2] for j in (5, 37, 133, 165, 130, 100)] == [(0, 0), (1, 0), (0, 1), (1, 1), (0, 1), (3, 0)]
    from ssv_amd import _lib
    assert (do.MATCH_MAX_S, do.MATCH_MAX_C) == (_lib.DENSE_MATCH_MAX_S, _lib.DENSE_MATCH_MAX_C)
    src = open(os.path.join(ROOT, "self-supervised-vision_amd", "csrc", "densecl.hip")).read()
    assert "if (s <= 128) SSV_DM(1, true); else SSV_DM(2, true);" in src and "const bool work = 32 * wave < s;" in src and "32 * (wave + 4 * t) + row" in src
    doc = forms.documented_labels()
    assert len(doc) == 9 and set(doc.values()) == {"ssv_dense_match"}
    used = {b for labels in forms.TARGETS.values() for b in labels.split()}
    assert set(doc) == used and set(forms.TARGETS) == {name for name in dir(forms) if name.startswith("test_")}


@pytest.mark.parametrize("seed", do.MATCH_SEEDS)
@pytest.mark.parametrize("case", do.FORM_MATCH_CASES, ids=do.match_id)
def test_match_form_cases_keep_the_fp32_reference_meaningful(case, seed):
    """As for MATCH_CASES: the fp32 oracle picks the fp64 arg-max in every cell and the smallest fp64 cosine gap is at least 1e-6 (planted copies count as their
    original; the NaN cell has no gap); and the conditions of the planted variants"""
    ins = do.make_match_case(case, seed)
    f1, f2 = ins[:2]
    b, s, c, variant = case
    eps = do.match_eps(case)
    assert f1.shape == f2.shape == (b, s, c) and len(ins) == (3 if variant == "eps" else 2) and (variant != "eps" or ins[2] == eps == 0.5)
    r64, r32 = do.dense_match(f1, f2, eps), do.dense_match(f1, f2, eps, dtype=torch.float32)
    gap = do.match_gap(case, r64)
    print(f"{do.match_id(case)} seed {seed}: smallest gap {gap:.3g}")
    assert torch.equal(r64["j"], r32["j"]) and gap >= 1e-6
    if variant == "signed":
        assert float(f1.min()) < 0.0 and float(f2.min()) < 0.0 and float(f2.abs().sum(dim=2).min()) > 0.0
    if variant == "perm":
        p = do.match_perm(case, seed)
        assert all(sorted(row) == list(range(s)) for row in p.tolist()) and torch.equal(r64["j"], p) and gap >= 0.1
        assert float((r64["sim"] - 1.0).abs().max()) < 1e-12
    if variant == "ties":
        for ref, dt in ((r64, torch.float64), (r32, torch.float32)):
            for copy, orig in do.TIES.items():
                assert torch.equal(ref["score"][0, :, copy].view(torch.int64 if dt == torch.float64 else torch.int32),
                                   ref["score"][0, :, orig].view(torch.int64 if dt == torch.float64 else torch.int32)), (copy, orig)
            assert [int(ref["j"][0, cell]) for cell in (0, 40, 1, 255)] == [5, 5, 100, 100]
            assert not bool(torch.isin(ref["j"][0], torch.tensor(list(do.TIES))).any())
    if variant == "eps":
        loose = do.dense_match(f1, f2, 1e-12)
        share = float((loose["j"] != r64["j"]).double().mean())
        print(f"{do.match_id(case)} seed {seed}: the clamp changes the arg-max in {100 * share:.1f} % of the cells")
        assert share >= 0.25 and not bool((r64["j"] % 2 == 0).any())
        assert float(f2[:, ::2].double().norm(dim=2).max()) < eps < float(f2[:, 1::2].double().norm(dim=2).min())
    if variant == "nan":
        n, i, ch = do.NAN_CELL
        assert bool(torch.isnan(f1[n, i, ch])) and int(torch.isnan(f1).sum()) == 1 and not bool(torch.isnan(f2).any())
        assert int(r64["idx"][n, i]) == n * s + 0 and bool(torch.isnan(r64["sim"][n, i])) and int(torch.isnan(r64["sim"]).sum()) == 1


def test_the_densecl_forms_accuracy_bounds_are_what_the_committed_report_implies():
    """FACTOR of tests/test_gpu_dense_nce_forms.py and of tests/test_gpu_dense_match_forms.py = the worst measured ratio of their family in
    profiles/densecl_forms_report.json rounded up to the next power of two, never above 8; every case, arithmetic and output is in the report; the older
    table's FACTOR is untouched"""
    import forms_report as fr
    import test_gpu_dense_match_forms as mforms
    import test_gpu_dense_nce_forms as qforms
    doc = json.load(open(os.path.join(ROOT, "profiles", "densecl_forms_report.json")))
    for forms, name, ids, outs in ((qforms, "dense_nce.forms", [do.case_id(c) for c in do.FORM_CASES], {"loss", "lse", "dq"}),
                                   (mforms, "dense_match.forms", [do.match_id(c) for c in do.FORM_MATCH_CASES], {"sim"})):
        fam = doc["families"][name]
        worst = max(fam["worst_e_ratio"], fam["worst_m_ratio"])
        assert worst <= 8.0 and fam["FLOOR"] == forms.FLOOR <= 16 * fr.U and forms.FACTOR == fr.next_pow2(worst) == fam["FACTOR"] == fam["FACTOR_implied"], name
        assert set(doc["cases"][name]) == {f"{i}[{a}]" for i in ids for a in ARITHS}
        assert all(set(t) == outs for t in doc["cases"][name].values())
    assert set(doc["match_cells"]) == set(doc["cases"]["dense_match.forms"]) and all(v["excused"] <= 0.01 * v["cells"] for v in doc["match_cells"].values())
    assert re.fullmatch(r"[0-9a-f]{16}", doc["source_sha16"]) and do.FACTOR == 8.0 and do.FLOOR == 2 * fr.U
