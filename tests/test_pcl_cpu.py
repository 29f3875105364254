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


# ---- the launch forms of tests/test_gpu_proto_nce_forms.py ------------------------------------------------------------------------------------------------------
ARITHS = ("bf16x3", "f32")


def test_plan_restatement_is_the_librarys():
    """pcl_oracle.plan against what the library exposes of its plan - the workspace size in both arithmetics - at every old and new case and at shapes around
    each threshold; and the dispatch lines it restates."""
    from ssv_amd import _lib
    assert (po.SLICE, po.MAX_SLICES, po.MAX_SEGS, po.FUSED_MAX_D) == (_lib.PROTO_NCE_SLICE, _lib.PROTO_NCE_MAX_SLICES, _lib.PROTO_NCE_MAX_SEGS, _lib.PROTO_NCE_FUSED_MAX_D)
    src, hdr = (open(os.path.join(ROOT, "self-supervised-vision_amd", "csrc", f)).read() for f in ("protonce.hip", "bank_softmax.h"))
    # the tile rule, the chunk rule and the <DT, KT> ladder are written once, in the header; the file names them
    assert "p.KT = (p.T == 1 || p.DT >= 3) ? 1 : 2;" in hdr and f"constexpr int CHUNK_ROWS = {po.CHUNK_ROWS};" in hdr and "CHUNK_ELEMS = 1ll << 25;" in hdr
    assert "if ((p).DT == 4) hipLaunchKernelGGL((KERNEL<4, 1>)" in hdr and "else if ((p).DT == 3) hipLaunchKernelGGL((KERNEL<3, 1>)" in hdr
    assert "banksm::plan_tiles(p, m, d);" in src and "p.cr = banksm::chunk_rows(p.kp, m);" in src and "SSV_FUSED_LADDER(pn_fused_k, p," in src
    lib = _lib.load()
    shapes = [c[:3] for c in po.cases() + po.FORM_CASES]
    shapes += [(m, d, (300, 300)) for m in (1, 32, 33, 64, 65, 1024, 1025, 8192) for d in (32, 64, 96, 128, 132, 160, 4)]
    shapes += [(40, 32, (k,)) for k in (po.SLICE * po.MAX_SLICES, po.SLICE * po.MAX_SLICES + 1, 1 << 20)] + [(2000, 36, (40000, 5))]
    for m, d, sizes in shapes:
        for arith in ARITHS:
            code = _lib.ARITH_BF16X3 if arith == "bf16x3" else _lib.ARITH_F32_MFMA
            p = po.plan(m, d, sizes, arith)
            assert lib.ssv_proto_nce_workspace_bytes(m, sum(sizes), d, len(sizes), code) == p["bytes"], (m, d, sizes, arith)
            assert p["fused"] == (arith == "bf16x3" and d % 32 == 0 and d <= po.FUSED_MAX_D)
            if p["fused"]:
                assert all(r % po.SLICE == 0 and -(-k // r) <= po.MAX_SLICES for k, r in zip(sizes, p["rows"])) and p["first"][-1] <= min(-(-sum(sizes) // po.SLICE) + len(sizes), po.MAX_SLICES * len(sizes))


def test_form_cases_reach_every_launch_form():
    """All the (DT, KT) instantiations the dispatch of ssv_proto_nce can launch - six: DT = 3 and 4 with one query tile, DT = 1 and 2 with one (T = 1) or two -
    over the old and the new tables, the new one bringing (3, 1); a segment with L > SLICE; eight segments; two unfused chunks; the unfused route under bf16x3 at a
    width that is a multiple of 32; and every label of the GPU file is reached by the case that names it."""
    import test_gpu_proto_nce_forms as forms
    inst = lambda cases: {(p["DT"], p["KT"]) for p in (po.plan(*c[:3], "bf16x3") for c in cases) if p["fused"]}
    assert inst(po.cases()) == {(1, 1), (1, 2), (2, 1), (2, 2), (4, 1)}, "the table of tests/test_gpu_proto_nce.py changed: revisit what the forms table must add"
    assert (3, 1) in inst(po.FORM_CASES) and inst(po.cases() + po.FORM_CASES) == {(1, 1), (1, 2), (2, 1), (2, 2), (3, 1), (4, 1)}
    new = [po.plan(*c[:3], "bf16x3") for c in po.FORM_CASES]
    assert any(p["fused"] and max(p["rows"]) > po.SLICE for p in new) and all(max(po.plan(*c[:3], "bf16x3").get("rows", [0])) <= po.SLICE for c in po.cases())
    assert max(len(c[2]) for c in po.FORM_CASES) == po.MAX_SEGS == 8 and max(len(c[2]) for c in po.cases()) == 3
    assert any(not p["fused"] and c[1] % 32 == 0 for c, p in zip(po.FORM_CASES, new))
    for arith in ARITHS:
        assert any(po.plan(*c[:3], arith).get("chunks") == 2 for c in po.FORM_CASES) and all(po.plan(*c[:3], arith).get("chunks", 1) == 1 for c in po.cases())
    assert any(not p["fused"] and p["chunks"] == 2 and p["kp"][0] == c[2][0] for c, p in zip(po.FORM_CASES, (po.plan(*c[:3], "f32") for c in po.FORM_CASES))) or \
        any(k % 16 == 0 for c in po.FORM_CASES for k in c[2]), "k % 16 == 0: pn_pad_k without a pad row"
    assert {c[2] for c in po.FORM_CASES} >= {(255,), (256,), (257,), po.EIGHT, (po.LONG,)} and {po.SLICE - 1, po.SLICE, po.SLICE + 1} <= set(po.EIGHT)
    assert len(set(po.FORM_CASES)) == len(po.FORM_CASES) and not set(po.FORM_CASES) & set(po.cases()) and set(po.FORM_ROUTES_AGREE) <= set(po.FORM_CASES)
    assert set(forms.CASE_LABELS) == set(po.FORM_CASES) and forms.ARITHS == ARITHS
    for case, labels in forms.CASE_LABELS.items():
        for arith, label in zip(ARITHS, labels):
            assert not label or forms.reaches(label, case, arith), (case, arith, label)
    doc = forms.documented_labels()
    assert len(doc) >= 13 and set(doc.values()) == {"ssv_proto_nce"}
    used = {b for labels in forms.TARGETS.values() for b in labels.split()}
    assert not set(doc) - used, f"documented branches without a case: {sorted(set(doc) - used)}"
    assert not used - set(doc), f"cases name undocumented branches: {sorted(used - set(doc))}"
    assert set(forms.TARGETS) == {name for name in dir(forms) if name.startswith("test_")}


@pytest.mark.parametrize("seed", po.FORM_SEEDS)
@pytest.mark.parametrize("case", po.FORM_CASES, ids=po.case_id)
def test_form_cases_keep_the_fp32_reference_meaningful(case, seed):
    """In fp64: the mean probability of the positive is below 0.9 and no score leaves [-60, 60]; the fp32 evaluation of dq is within 7e-7 of it (e)"""
    ins = po.make_case(case, seed)
    q, protos, inv_phi, labels, seg_end = ins
    m, d, sizes, variant = case
    assert q.shape == (m, d) and protos.shape == (sum(sizes), d) and labels.shape == (len(sizes), m) and seg_end[-1] == sum(sizes)
    for s, k in enumerate(sizes):
        assert 0 <= int(labels[s].min()) and int(labels[s].max()) < k
    ref, r32 = po.proto_nce(*ins), po.proto_nce(*ins, dtype=torch.float32)
    e = po.errs(r32["dq"], ref["dq"])[0]
    print(f"{po.case_id(case)} seed {seed}: pos {ref['pos']:.3g} smax {ref['smax']:.3g} e(ref32) of dq {e:.3g}")
    assert ref["pos"] < 0.9, ref["pos"]
    assert ref["smax"] <= 60.0, ref["smax"]
    assert float(ref["dq"].abs().max()) > 0.0 and float(ref["loss"]) > 0.0
    assert e <= 7e-7, e
    if variant == "late":
        sc = (q.double() @ protos.double()[seg_end[-2] if len(seg_end) > 1 else 0:].T) * inv_phi.double()[seg_end[-2] if len(seg_end) > 1 else 0:]
        assert bool((sc.argmax(dim=1) == sc.shape[1] - 1).all())
    if variant == "dup":
        assert torch.equal(protos[255], protos[256]) and inv_phi[255] == inv_phi[256]


def test_the_forms_accuracy_bound_is_what_the_committed_report_implies():
    """FACTOR of tests/test_gpu_proto_nce_forms.py = the worst measured ratio of profiles/lookup_loss_forms_report.json rounded up to the next power of two, never
    above 8; every case and both arithmetics are in the report; the older table's FACTOR is untouched."""
    import json
    import forms_report as fr
    import test_gpu_proto_nce_forms as forms
    doc = json.load(open(os.path.join(ROOT, "profiles", "lookup_loss_forms_report.json")))
    fam = doc["families"]["proto_nce.forms"]
    worst = max(fam["worst_e_ratio"], fam["worst_m_ratio"])
    assert worst <= 8.0 and fam["FLOOR"] == forms.FLOOR == po.FLOOR and forms.FACTOR == fr.next_pow2(worst) == fam["FACTOR"]
    assert set(doc["cases"]["proto_nce.forms"]) == {f"{po.case_id(c)}[{a}]" for c in po.FORM_CASES for a in ARITHS}
    assert all(set(t) == {"loss", "lse", "dq"} for t in doc["cases"]["proto_nce.forms"].values()) and re.fullmatch(r"[0-9a-f]{16}", doc["source_sha16"])
    assert po.FACTOR == 4.0
