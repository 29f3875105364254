"""CPU: the NNCLR oracle (tests/nnclr_oracle.py) against an independent restatement and against its own float32 evaluation, the near-tie share of the lookup
cases the GPU tests run, and the GPU-free surface of the feature: the command line, the two configs, the two entry points, the slice rule."""
import os
import re

import numpy as np
import pytest
import torch
import yaml

import nnclr_oracle as no

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "self-supervised-vision_amd", "configs")
HEADER = os.path.join(ROOT, "include", "ssv_hip.h")
COND = 1e-3                     # tests/test_gpu_loss_kernels.py rule (b)
LOSS_RUNS = [(b, d, n, t) for b, d, n in no.LOSS_SHAPES for t in no.TEMPERATURES]


def test_cli_resolves_nnclr_and_still_refuses_the_unbuilt():
    from ssv_amd import main as cli
    from ssv_amd.models.base import TwoViewTrainer
    cls = cli.trainer_class("nnclr")
    assert cls.__name__ == "NNCLR" and issubclass(cls, TwoViewTrainer)
    assert cls.algo == "nnclr" and cls.graph_safe is True and cls.graph_inputs == ("aug_1", "aug_2")
    assert cli.ALGORITHMS["nnclr"] == ("nnclr", "NNCLR")
    for name in ("deep_cluster", "swav", "sela"):
        assert cli.ALGORITHMS[name] is None
        with pytest.raises(NotImplementedError):
            cli.trainer_class(name)
    assert cli.parse(["-c", "x.yaml", "-a", "nnclr", "-m", "resnet18", "-t", "train"])["algo"] == "nnclr"


@pytest.mark.parametrize("fname,size,queue", [("nnclr.yaml", 32, 16384), ("nnclr_r50_224_synthetic.yaml", 224, 98304)])
def test_configs_parse(fname, size, queue):
    from ssv_amd.utils import augmentations, losses
    cfg = yaml.safe_load(open(os.path.join(CONFIGS, fname)))
    batch, proj = cfg["data"]["batch_size"], cfg["proj_dim"]
    assert (batch, proj, cfg["proj_hidden_dim"], cfg["pred_hidden_dim"], cfg["queue_size"]) == (512, 256, 2048, 4096, queue)
    assert proj % 32 == 0 and cfg["queue_size"] >= 2 * batch
    assert cfg["loss_fn"] == {"temperature": 0.1}
    simclr = yaml.safe_load(open(os.path.join(CONFIGS, "simclr.yaml" if size == 32 else "simclr_r50_224_synthetic.yaml")))
    assert cfg["optimizer"] == simclr["optimizer"] and cfg["scheduler"] == simclr["scheduler"] and cfg["encoder"] == simclr["encoder"]
    for split in ("train", "test"):
        assert augmentations.get_transform(cfg["data"]["transforms"][split]) is not None
    assert cfg["data"]["transforms"]["train"]["random_resized_crop"]["size"] == [size, size]
    fn = losses.NnclrLoss(**cfg["loss_fn"])
    assert fn.temperature == 0.1 and fn.last_idx is None


def test_loss_module_refuses_bad_arguments():
    from ssv_amd.utils import losses
    fn = losses.NnclrLoss()
    z, bank = torch.zeros(8, 32), torch.zeros(16, 32)
    for args in ((torch.zeros(8), z, z, z, bank), (z, z, z, torch.zeros(4, 32), bank), (z, z, z, z, torch.zeros(16, 64)), (z, z, z, z, bank, 17), (z, z, z, z, bank, 0),
                 (torch.zeros(8, 30),) * 4 + (torch.zeros(16, 30),), (torch.zeros(4097, 32),) * 4 + (bank,)):
        with pytest.raises(ValueError):
            fn(*args)
    with pytest.raises(ValueError):
        losses.NnclrLoss(temperature=0.0)


def test_entry_points_are_declared_and_bound():
    import ctypes as C
    from ssv_amd import _lib
    text = open(HEADER).read()
    assert re.search(r"size_t ssv_nn_lookup_workspace_bytes\(int32_t m, int64_t n, int32_t d, int32_t arithmetic\);", text)
    assert re.search(r"int ssv_nn_lookup\(int32_t m, int64_t n, int32_t d, const float\* queries, const float\* bank, float out_scale, float\* nn, int32_t\* idx, "
                     r"float\* sim,\s+int32_t arithmetic, void\* ws, size_t ws_bytes, void\* stream\);", text)
    vp, i32, i64, f32, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_size_t
    assert _lib.SIGNATURES["ssv_nn_lookup_workspace_bytes"] == (sz, [i32, i64, i32, i32])
    assert _lib.SIGNATURES["ssv_nn_lookup"] == (C.c_int, [i32, i64, i32, vp, vp, f32, vp, vp, vp, i32, vp, sz, vp])
    lib = _lib.load()
    assert _lib.ABI_VERSION == 124 and lib.ssv_version() == 124
    for arith in (_lib.ARITH_F32_MFMA, _lib.ARITH_BF16X3):
        assert lib.ssv_nn_lookup_workspace_bytes(1024, 98304, 256, arith) > 0
        for m, n, d in ((0, 16, 32), (-1, 16, 32), (8193, 16, 32), (8, 0, 32), (8, 1 << 31, 32), (8, 16, 0), (8, 16, 30), (8, 16, 8196)):
            assert lib.ssv_nn_lookup_workspace_bytes(m, n, d, arith) == 0, (m, n, d)
    assert lib.ssv_nn_lookup_workspace_bytes(8, 16, 32, 3) == 0
    # the fused route keeps no S: at the paper's shape its workspace is the partials and the queries' planes, a few MB
    assert lib.ssv_nn_lookup_workspace_bytes(1024, 98304, 256, _lib.ARITH_BF16X3) < 8 << 20
    assert lib.ssv_nn_lookup(8, 16, 32, None, None, 1.0, None, None, None, _lib.ARITH_BF16X3, None, 0, None) == -1
    assert lib.ssv_last_error().decode().startswith("ssv_nn_lookup:")


def test_slice_rule_is_the_headers():
    from ssv_amd import _lib, ops
    text = open(HEADER).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (SSV_NN_LOOKUP_\w+) (\d+)", text)}
    assert defs == {"SSV_NN_LOOKUP_MAX_M": _lib.NN_LOOKUP_MAX_M, "SSV_NN_LOOKUP_FUSED_MAX_D": _lib.NN_LOOKUP_FUSED_MAX_D, "SSV_NN_LOOKUP_SLICE": _lib.NN_LOOKUP_SLICE,
                    "SSV_NN_LOOKUP_MAX_SLICES": _lib.NN_LOOKUP_MAX_SLICES}
    assert _lib.NN_LOOKUP_FUSED_MAX_D >= 256 and _lib.NN_LOOKUP_FUSED_MAX_D % 32 == 0 and _lib.NN_LOOKUP_SLICE % 128 == 0
    s = _lib.NN_LOOKUP_SLICE
    assert [ops.nn_lookup_slice_rows(n) for n in (1, s, s + 1, 98304, s * 4096, s * 4096 + 1, (1 << 31) - 1)] == [s, s, s, s, s, 2 * s, 1024 * s]
    # the partials of the fused route are sized by that rule: slices x queries (padded to 32) x (score, index)
    lib = _lib.load()
    for m, n, d in ((1024, 98304, 256), (64, 70000, 128), (40, s * 4096 + 1, 32)):
        slices = -(-n // ops.nn_lookup_slice_rows(n))
        planes = 3 * (-(-d // 64) * 4) * -(-m // 32) * 1024
        up = lambda v: (v + 255) // 256 * 256
        assert lib.ssv_nn_lookup_workspace_bytes(m, n, d, _lib.ARITH_BF16X3) == 2 * up(slices * (-(-m // 32) * 32) * 4) + planes
    with pytest.raises(_lib.SsvError):
        ops.nn_lookup_slice_rows(0)


# ---- the oracle -------------------------------------------------------------------------------------------------------------------------------------------------
def _loss_case(b, d, n, t):
    z1, z2, p1, p2, bank = no.loss_inputs(b, d, n)
    zq = torch.cat((z1, z2)).double()
    zq = zq / zq.norm(dim=1, keepdim=True)
    idx = torch.from_numpy(no.scores(zq.float().numpy(), bank[:n].numpy()).argmax(1))
    a = no.neighbours(bank, idx, t)
    return p1, p2, a[:b], a[b:]


@pytest.mark.parametrize("b,d,n,t", LOSS_RUNS)
def test_oracle_agrees_with_an_independent_restatement(b, d, n, t):
    p1, p2, a1, a2 = _loss_case(b, d, n, t)
    ref, other = no.loss_reference(p1, p2, a1, a2, torch.float64), no.restated(p1, p2, a1, a2, torch.float64)
    for k in ("loss", "dp1", "dp2"):
        assert float(ref[k].abs().max()) > 0
        assert float((ref[k] - other[k]).abs().max()) <= 1e-12 * float(ref[k].abs().max()), k
    for got, want in ((0.5 * no.closed_form(p1.double(), a2.double()), ref["dp1"]), (0.5 * no.closed_form(p2.double(), a1.double()), ref["dp2"])):
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("b,d,n,t", LOSS_RUNS)
def test_reference_is_well_conditioned(b, d, n, t):
    p1, p2, a1, a2 = _loss_case(b, d, n, t)
    r64, r32 = no.loss_reference(p1, p2, a1, a2, torch.float64), no.loss_reference(p1, p2, a1, a2, torch.float32)
    for k in r64:
        e, m = no.errors(r32[k], r64[k])
        assert e < COND and m < COND, (k, e, m)


@pytest.mark.parametrize("name", list(no.LOOKUP_CASES))
def test_near_ties_stay_under_the_cap(name):
    """The GPU test excuses a row whose fp64 margin lies below tau_i from carrying the exact arg-max; the cap keeps that from hollowing the test out."""
    r = no.lookup_reference(name)
    c = no.LOOKUP_CASES[name]
    share = float(r["excused"].mean())
    print(f"{name}: {100 * share:.2f} % of {c.m} queries within tau of a tie (smallest margin {r['margin'].min():.3g}, tau {r['tau'].max():.3g})")
    assert r["s"].shape == (c.m, c.n) and np.isfinite(r["s"]).all()
    assert share <= no.MAX_EXCUSED
    q, b = no.lookup_inputs(name)
    for x in (q, b):
        assert np.abs(np.sqrt((x.astype(np.float64) ** 2).sum(1)) - 1).max() < 1e-6


# ---- the launch forms of tests/test_gpu_nn_lookup_forms.py ------------------------------------------------------------------------------------------------------
ARITHS = ("bf16x3", "f32")


def _code(arith):
    from ssv_amd import _lib
    return _lib.ARITH_BF16X3 if arith == "bf16x3" else _lib.ARITH_F32_MFMA


def test_lookup_plan_restatement_is_the_librarys():
    """nnclr_oracle.lookup_plan against what the library exposes of its plan: the workspace size in both arithmetics (slices x padded queries and the queries'
    planes, or the chunk of S) and the rows of a slice, at every old and new case and at shapes around each threshold; and the dispatch line it restates."""
    from ssv_amd import _lib, ops
    assert (no.SLICE, no.MAX_SLICES, no.FUSED_MAX_D) == (_lib.NN_LOOKUP_SLICE, _lib.NN_LOOKUP_MAX_SLICES, _lib.NN_LOOKUP_FUSED_MAX_D)
    src = open(os.path.join(ROOT, "self-supervised-vision_amd", "csrc", "nnlookup.hip")).read()
    assert "if (p.T == 1) SSV_NN(1); else if (p.T == 2) SSV_NN(2); else if (p.T <= 4) SSV_NN(4); else SSV_NN(8);" in src
    assert f"constexpr int CHUNK_ROWS = {no.CHUNK_ROWS};" in src and "PART_ELEMS = 1ll << 26, MAX_PART_COLS = 65536;" in src
    lib = _lib.load()
    s, cap = no.SLICE, no.SLICE * no.MAX_SLICES
    shapes = list(no.LOOKUP_SHAPES + no.FORM_LOOKUP_SHAPES)
    shapes += [(m, 700, 64) for m in (1, 32, 33, 64, 65, 96, 97, 128, 129, 8192)] + [(40, n, 32) for n in (1, s, s + 1, cap, cap + 1, 2 * cap, 2 * cap + 1)]
    shapes += [(1025, 70000, d) for d in (4, 1020, 1024, 1028, 8192)]
    for m, n, d in shapes:
        for arith in ARITHS:
            p = no.lookup_plan(m, n, d, arith)
            assert lib.ssv_nn_lookup_workspace_bytes(m, n, d, _code(arith)) == p["bytes"], (m, n, d, arith)
            assert p["fused"] == (arith == "bf16x3" and d % 32 == 0 and d <= no.FUSED_MAX_D)
            if p["fused"]:
                assert p["L"] == ops.nn_lookup_slice_rows(n) and (p["P"] - 1) * p["L"] < n <= p["P"] * p["L"] and p["P"] <= no.MAX_SLICES
                assert p["KT"] in (1, 2, 4, 8) and (p["blocks"] - 1) * p["KT"] < p["T"] <= p["blocks"] * p["KT"]


def test_form_cases_reach_every_launch_form():
    """The forms the issue lists, from the restated plan: all four KT of nn_fused_k over the old and the new tables (the new one brings KT = 4, with T = 3 and with
    T = 4), both routes under bf16x3 at d % 32 != 0 and at d > SSV_NN_LOOKUP_FUSED_MAX_D, nch = 16, L > SLICE, a ragged last block of KT = 8, two query chunks; and
    every label of the GPU file is reached by the case that names it."""
    import test_gpu_nn_lookup_forms as forms
    new = [no.lookup_plan(m, n, d, "bf16x3") for m, n, d in no.FORM_LOOKUP_SHAPES]
    old = [no.lookup_plan(m, n, d, "bf16x3") for m, n, d in no.LOOKUP_SHAPES]
    assert {p["KT"] for p in old if p["fused"]} == {1, 2, 8}, "the table of tests/test_gpu_nnclr.py changed: revisit what the forms table must add"
    assert {p["KT"] for p in new + old if p["fused"]} == {1, 2, 4, 8}
    assert {p["T"] for p in new if p["fused"] and p["KT"] == 4} == {3, 4}
    assert {p["fused"] for p in new} == {True, False}
    unfused = [(m, n, d) for (m, n, d), p in zip(no.FORM_LOOKUP_SHAPES, new) if not p["fused"]]
    assert any(d % 32 != 0 and d < no.FUSED_MAX_D for _, _, d in unfused) and any(d % 32 == 0 and d > no.FUSED_MAX_D for _, _, d in unfused)
    assert max(p["nch"] for p in new if p["fused"]) == no.FUSED_MAX_D // 64 == 16 and max(p["nch"] for p in old) < 16
    assert max(p["L"] for p in new if p["fused"]) == 2 * no.SLICE and all(p["L"] == no.SLICE for p in old)
    assert any(p["fused"] and p["KT"] == 8 and p["T"] % 8 == 1 for p in new)
    for arith in ARITHS:
        assert any(no.lookup_plan(m, n, d, arith).get("chunks") == 2 for m, n, d in no.FORM_LOOKUP_SHAPES)
        assert all(no.lookup_plan(m, n, d, arith).get("chunks", 1) == 1 for m, n, d in no.LOOKUP_SHAPES)
    assert set(forms.CASE_LABELS) == {f"{m}x{n}x{d}" for m, n, d in no.FORM_LOOKUP_SHAPES}
    for (m, n, d) in no.FORM_LOOKUP_SHAPES:
        for arith, label in zip(forms.ARITHS, forms.CASE_LABELS[f"{m}x{n}x{d}"]):
            assert not label or forms.reaches(label, m, n, d, arith), (m, n, d, arith, label)
    assert forms.ARITHS == ARITHS
    kinds = {(c.m, c.n, c.d): set() for c in no.FORM_LOOKUP_CASES.values()}
    for c in no.FORM_LOOKUP_CASES.values():
        kinds[(c.m, c.n, c.d)].add(c.kind)
    assert all(k == ({"gauss"} if n == no.FORM_BIG_N else set(no.KINDS)) for (_, n, _), k in kinds.items()) and set(kinds) == set(no.FORM_LOOKUP_SHAPES)
    assert not set(no.FORM_LOOKUP_CASES) & set(no.LOOKUP_CASES)


def test_forms_table_covers_every_documented_branch():
    import test_gpu_nn_lookup_forms as forms
    doc = forms.documented_labels()
    assert len(doc) >= 13 and set(doc.values()) == {"ssv_nn_lookup"}
    used = {b for labels in forms.TARGETS.values() for b in labels.split()}
    assert not set(doc) - used, f"documented branches without a case: {sorted(set(doc) - used)}"
    assert not used - set(doc), f"cases name undocumented branches: {sorted(used - set(doc))}"
    assert set(forms.TARGETS) == {name for name in dir(forms) if name.startswith("test_")}


def test_the_committed_forms_report_holds_every_lookup_run():
    """profiles/lookup_loss_forms_report.json, "lookup": every case in both arithmetics at both scales, and the planted case; no row off the fp64 arg-max beyond
    the excused ones, sim within tau"""
    import json
    doc = json.load(open(os.path.join(ROOT, "profiles", "lookup_loss_forms_report.json")))
    runs = doc["lookup"]
    assert set(runs) == {f"{name}[{a}] scale {s}" for name in list(no.FORM_LOOKUP_CASES) + ["planted"] for a in ARITHS for s in (1, 10)}
    for name, r in runs.items():
        assert r["off_the_fp64_argmax"] <= r["excused"] <= no.MAX_EXCUSED * r["rows"] and r["worst_sim_error_over_tau"] <= 1.0, name
    assert re.fullmatch(r"[0-9a-f]{16}", doc["source_sha16"])


@pytest.mark.parametrize("name", list(no.FORM_LOOKUP_CASES))
def test_form_cases_stay_under_the_near_tie_cap(name):
    r = no.lookup_reference(name)
    c = no.FORM_LOOKUP_CASES[name]
    share = float(r["excused"].mean())
    print(f"{name}: {100 * share:.2f} % of {c.m} queries within tau of a tie (smallest margin {r['margin'].min():.3g}, tau {r['tau'].max():.3g})")
    assert r["s"].shape == (c.m, c.n) and np.isfinite(r["s"]).all()
    assert share <= no.MAX_EXCUSED
    if c.n == no.FORM_BIG_N:
        assert not r["excused"].any(), "with 8 queries one excused row is 12.5 %"
    q, b = no.lookup_inputs(name)
    for x in (q, b):
        assert np.abs(np.sqrt((x.astype(np.float64) ** 2).sum(1)) - 1).max() < 1e-6
