"""CPU: the host side of the PCL trainer (models/pcl.py, csrc/protonce.hip) - the oracle against a case worked by hand, the command line, the configs, the ABI
surface and the workspace sizing, and the two conditions the kernel tests' case table must meet so that its fp32 reference means something."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch
import yaml

import pcl_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "self-supervised-vision_amd", "configs")
HEADER = os.path.join(ROOT, "include", "ssv_hip.h")


def test_oracle_agrees_with_a_hand_written_two_prototype_case():
    """q = (1, 0), prototypes (1, 0) and (0, 1) with 1 / phi = 2 and 3, label 0: s = (2, 0), lse = log(e^2 + 1), p = (e^2, 1) / (e^2 + 1),
    dq = p_0 * 2 * c_0 + p_1 * 3 * c_1 - 2 * c_0 = (2 (p_0 - 1), 3 p_1)"""
    q = torch.tensor([[1.0, 0.0]])
    protos = torch.tensor([[1.0, 0.0], [0.0, 1.0]])
    out = po.proto_nce(q, protos, torch.tensor([2.0, 3.0]), torch.tensor([[0]], dtype=torch.int32), (2,))
    lse = math.log(math.exp(2.0) + 1.0)
    p0, p1 = math.exp(2.0 - lse), math.exp(-lse)
    assert abs(float(out["lse"][0, 0]) - lse) < 1e-14 and abs(float(out["loss"]) - (lse - 2.0)) < 1e-14
    assert torch.allclose(out["dq"], torch.tensor([[2.0 * (p0 - 1.0), 3.0 * p1]], dtype=torch.float64), atol=1e-14, rtol=0)
    assert abs(out["pos"] - p0) < 1e-14 and out["smax"] == 2.0
    # two segments of one prototype each: every lse is the score, the loss and the gradient vanish
    one = po.proto_nce(q, protos, torch.tensor([2.0, 3.0]), torch.tensor([[0], [0]], dtype=torch.int32), (1, 2))
    assert float(one["loss"]) == 0.0 and float(one["dq"].abs().max()) == 0.0 and one["lse"].flatten().tolist() == [2.0, 0.0]
    # the float32 evaluation runs the same lines
    assert po.proto_nce(q, protos, torch.tensor([2.0, 3.0]), torch.tensor([[0]], dtype=torch.int32), (2,), torch.float32)["dq"].dtype == torch.float32


def test_concentration_oracle_on_a_hand_written_case():
    """three clusters: two members at distances 1 and 3 (phi = 2 / log 12), four members at distance 2 (phi = 2 / log 14), one member (takes the largest)"""
    dist = torch.tensor([1.0, 9.0, 4.0, 4.0, 4.0, 4.0, 25.0])
    labels = torch.tensor([0, 0, 1, 1, 1, 1, 2], dtype=torch.int32)
    counts = torch.tensor([2, 4, 1], dtype=torch.int32)
    raw = np.array([2.0 / math.log(12.0), 2.0 / math.log(14.0), 2.0 / math.log(12.0)])
    raw = np.clip(raw, np.percentile(raw, 10), np.percentile(raw, 90))
    want = 0.2 * raw / raw.mean()
    got = po.cluster_concentration(dist, labels, counts, alpha=10.0, temperature=0.2)
    assert np.allclose(got, want, rtol=1e-15, atol=0) and abs(got.mean() - 0.2) < 1e-15


def test_cli_resolves_pcl_and_still_refuses_the_unbuilt():
    from ssv_amd import main as cli
    from ssv_amd.models.base import TwoViewTrainer
    from ssv_amd.models.moco import MoCo
    cls = cli.trainer_class("pcl")
    assert cls.__name__ == "PCL" and issubclass(cls, TwoViewTrainer) and issubclass(cls, MoCo)
    assert cls.algo == "pcl" and cls.graph_safe is True and cls.graph_inputs == ("aug_1", "aug_2", "index")
    assert cli.ALGORITHMS["pcl"] == ("pcl", "PCL")
    for name in ("deep_cluster", "swav", "sela"):
        assert cli.ALGORITHMS[name] is None
        with pytest.raises(NotImplementedError):
            cli.trainer_class(name)
    assert cli.parse(["-c", "x.yaml", "-a", "pcl", "-m", "resnet18", "-t", "train"])["algo"] == "pcl"


@pytest.mark.parametrize("fname", ["pcl.yaml", "pcl_r18_32_synthetic.yaml"])
def test_configs_parse(fname):
    from ssv_amd import _lib
    from ssv_amd.utils import augmentations, losses
    cfg = yaml.safe_load(open(os.path.join(CONFIGS, fname)))
    block = cfg["pcl"]
    assert block["num_clusters"] == [250, 500, 1000] and len(block["num_clusters"]) <= _lib.PROTO_NCE_MAX_SEGS and max(block["num_clusters"]) <= _lib.KMEANS_MAX_K
    assert sorted(block) == ["alpha", "niter", "nredo", "num_clusters", "seed", "temperature", "warmup_epochs"]
    assert cfg["proj_dim"] == 128 and cfg["proj_dim"] % 32 == 0 and cfg["proj_dim"] <= _lib.PROTO_NCE_FUSED_MAX_D          # the shipped width takes the fused kernel
    assert cfg["loss_fn"] == {"normalize": True, "temperature": 0.07} and cfg["encoder"] == {"reduce_bottom_conv": True}
    moco = yaml.safe_load(open(os.path.join(CONFIGS, "moco.yaml")))
    assert cfg["data"]["transforms"] == moco["data"]["transforms"] and cfg["optimizer"] == moco["optimizer"]
    assert ("synthetic" in cfg["data"]) == ("synthetic" in fname)
    if "synthetic" in cfg["data"]:
        assert cfg["data"]["synthetic"]["num_train"] >= max(block["num_clusters"]) and cfg["data"]["batch_size"] == 512
    for split in ("train", "test"):
        assert augmentations.get_transform(cfg["data"]["transforms"][split]) is not None
    assert losses.MocoLoss(**cfg["loss_fn"]).temperature == 0.07 and losses.ProtoNceLoss(cfg["loss_fn"]["normalize"]).last_flag is None


def test_entry_points_are_declared_and_bound():
    from ssv_amd import _lib
    hdr = open(HEADER).read()
    vp, i32, i64, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t
    want = {"ssv_proto_nce_workspace_bytes": (sz, [i32, i64, i32, i32, i32]),
            "ssv_proto_nce": (C.c_int, [i32, i32, i32, C.POINTER(C.c_int64), vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, sz, vp])}
    for name, sig in want.items():
        assert re.search(rf"^(size_t|int) {name}\(", hdr, re.M), f"{name} is not declared in include/ssv_hip.h"
        assert _lib.SIGNATURES[name] == sig
        assert hasattr(_lib.load(), name)
    for macro, value in (("SSV_PROTO_NCE_MAX_M", _lib.PROTO_NCE_MAX_M), ("SSV_PROTO_NCE_MAX_SEGS", _lib.PROTO_NCE_MAX_SEGS), ("SSV_PROTO_NCE_FUSED_MAX_D", _lib.PROTO_NCE_FUSED_MAX_D),
                         ("SSV_PROTO_NCE_SLICE", _lib.PROTO_NCE_SLICE), ("SSV_PROTO_NCE_MAX_SLICES", _lib.PROTO_NCE_MAX_SLICES)):
        assert re.search(rf"^#define {macro} {value}$", hdr, re.M), macro
    assert _lib.PROTO_NCE_FUSED_MAX_D >= 128 and _lib.PROTO_NCE_FUSED_MAX_D == po.FUSED_MAX_D and _lib.PROTO_NCE_SLICE == po.SLICE
    assert _lib.ABI_VERSION == 124 and _lib.load().ssv_version() == 124
    src = open(os.path.join(ROOT, "self-supervised-vision_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bprotonce\.hip\b", src, re.M)


REFUSED_SHAPES = [(0, 100, 128, 1), (8193, 100, 128, 1), (16, 100, 128, 0), (16, 100, 128, 9), (16, 2, 128, 3), (16, 0, 128, 1), (16, 1 << 31, 128, 1), (16, 100, 126, 1),
                  (16, 100, 0, 1), (16, 100, 8196, 1)]                  # (m, ktot, d, segs)


def test_workspace_sizing_and_null_refusals():
    from ssv_amd import _lib
    lib = _lib.load()
    for arith in (_lib.ARITH_BF16X3, _lib.ARITH_F32_MFMA):
        for shape in REFUSED_SHAPES:
            assert lib.ssv_proto_nce_workspace_bytes(*shape, arith) == 0, shape
        assert lib.ssv_proto_nce_workspace_bytes(512, 1750, 128, 3, arith) > 0 and lib.ssv_proto_nce_workspace_bytes(1, 1, 4, 1, arith) > 0
        assert lib.ssv_proto_nce_workspace_bytes(8192, (1 << 31) - 1, 8192, 8, arith) > 0
    assert lib.ssv_proto_nce_workspace_bytes(512, 1750, 128, 3, 5) == 0                     # no such arithmetic
    # the fused route keeps (max, sum, acc[d]) per quarter slice and query: more slices, more workspace; the unfused route keeps a chunk of S
    assert lib.ssv_proto_nce_workspace_bytes(64, 4096, 128, 1, _lib.ARITH_BF16X3) > lib.ssv_proto_nce_workspace_bytes(64, 256, 128, 1, _lib.ARITH_BF16X3)
    assert lib.ssv_proto_nce_workspace_bytes(64, 4096, 36, 1, _lib.ARITH_BF16X3) == lib.ssv_proto_nce_workspace_bytes(64, 4096, 36, 1, _lib.ARITH_F32_MFMA)
    lib.ssv_last_error.restype = C.c_char_p
    ends = (C.c_int64 * 1)(100)
    assert lib.ssv_proto_nce(16, 128, 1, ends, None, None, None, None, None, None, None, None, _lib.ARITH_BF16X3, None, 0, None) == -1
    assert lib.ssv_last_error().decode().startswith("ssv_proto_nce:")
    assert lib.ssv_proto_nce(16, 128, 1, None, None, None, None, None, None, None, None, None, _lib.ARITH_BF16X3, None, 0, None) == -1
    assert lib.ssv_last_error().decode().startswith("ssv_proto_nce:")


def test_ops_and_loss_refuse_host_tensors_and_bad_shapes():
    from ssv_amd import _lib, ops
    from ssv_amd.utils import losses
    q, c, ip, lab = torch.zeros(4, 8), torch.zeros(6, 8), torch.ones(6), torch.zeros(1, 4, dtype=torch.int32)
    with pytest.raises(_lib.SsvError):
        ops.proto_nce(q, c, ip, lab, (6,))                                # CPU tensors: no fallback
    fn = losses.ProtoNceLoss()
    for bad_q, bad_c in ((torch.zeros(4, 6), torch.zeros(6, 6)), (torch.zeros(4, 8), torch.zeros(6, 12)), (torch.zeros(8), c), (torch.zeros(8193, 8), c)):
        with pytest.raises(ValueError):
            fn(bad_q, bad_c, ip, lab, (6,))
    assert ops.proto_nce_route(128) == ("fused" if ops.ARITHMETIC == "bf16x3" else "unfused")
    assert ops.proto_nce_route(36) == "unfused" and ops.proto_nce_route(160) == "unfused"
    with ops.arithmetic("f32"):
        assert ops.proto_nce_route(128) == "unfused"


def test_loss_module_is_single_process(monkeypatch):
    from ssv_amd import distributed as hdist
    from ssv_amd.utils import losses
    monkeypatch.setattr(hdist, "is_on", lambda: True)
    with pytest.raises(NotImplementedError):
        losses.ProtoNceLoss()(torch.zeros(4, 8), torch.zeros(6, 8), torch.ones(6), torch.zeros(1, 4, dtype=torch.int32), (6,))


def test_case_table_covers_the_mechanisms():
    cases = po.cases()
    assert len(set(cases)) == len(cases)
    assert {c[0] for c in cases} == {1, 33, 70}
    assert {c[1] for c in cases} == {32, 64, 128, po.FUSED_MAX_D, 4, 36}
    assert {c[2] for c in cases} >= {(31,), (33,), (513,), (7, 33, 600), (1, 33)}
    assert 2 * po.SLICE < 513 <= 2 * po.SLICE + 32                         # a segment just above two slices
    assert 600 > 2 * po.SLICE and 7 + 33 + po.SLICE < 640                  # a slice boundary inside the last of three segments
    assert {c[3] for c in cases} == {"plain", "dup", "late"}
    for case in cases:
        q, protos, inv_phi, labels, seg_end = po.make_case(case)
        m, d, sizes, variant = case
        assert q.shape == (m, d) and protos.shape == (sum(sizes), d) and labels.shape == (len(sizes), m) and seg_end[-1] == sum(sizes)
        assert 2.0 <= float(inv_phi.min()) and float(inv_phi.max()) <= 20.0 + 1e-5
        for s, k in enumerate(sizes):
            assert 0 <= int(labels[s].min()) and int(labels[s].max()) < k
            if m >= 33:
                assert 0 in labels[s].tolist() and k - 1 in labels[s].tolist()
                assert k <= 32 or any((k - 1) // 32 * 32 <= v for v in labels[s].tolist())
        if variant == "dup":
            assert torch.equal(protos[255], protos[256]) and inv_phi[255] == inv_phi[256]


@pytest.mark.parametrize("case", po.cases(), ids=po.case_id)
def test_case_table_keeps_the_fp32_reference_meaningful(case):
    """In fp64: the mean probability of the positive is below 0.9 (dq is no cancellation) and no score leaves [-60, 60]"""
    q, protos, inv_phi, labels, seg_end = po.make_case(case)
    ref = po.proto_nce(q, protos, inv_phi, labels, seg_end)
    assert ref["pos"] < 0.9, ref["pos"]
    assert ref["smax"] <= 60.0, ref["smax"]
    assert float(ref["dq"].abs().max()) > 0.0 and float(ref["loss"]) > 0.0
    if case[3] == "late":                                                  # the largest score of every query is the last prototype's
        sc = (q.double() @ protos.double()[seg_end[-2]:].T) * inv_phi.double()[seg_end[-2]:]
        assert bool((sc.argmax(dim=1) == sc.shape[1] - 1).all())
