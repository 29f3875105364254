"""CPU: what the launch-form tests of csrc/augment.hip (tests/test_gpu_augment_forms.py) rest on, held without a GPU - the entry points exist, the restated plan
of tests/augment_forms_oracle.py is the source's, every case of the tables has the property its label claims, Pillow agrees bit for bit with the restatement on
every pixel case, the crop draws take every branch and sit nowhere near a decision boundary, the colour cases reach every branch of the HSV round trip and both
clip ends of the blend, every refusal is decided by an SSV_REQUIRE before anything is launched, and each deliberately wrong variant of the restatement (MUTANTS)
changes the result of a case of the label it belongs to - so the GPU file would notice that mistake in a kernel."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import augment_forms_oracle as ao
import blur_oracle as bo
from oracle import augment as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "self-supervised-vision_amd", "csrc", "augment.hip")).read()
HEADER = open(os.path.join(ROOT, "include", "ssv_hip.h")).read()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def by_label(label):
    return [c for c in ao.PIXEL_CASES if c.label == label]


# ---- entry points and plan ------------------------------------------------------------------------------------------------------------------------------------------
def test_every_entry_point_is_still_spelled_that_way():
    import test_gpu_augment_forms as forms
    from ssv_amd import _lib
    assert len(ao.ENTRY_POINTS) == 8 == len(set(ao.ENTRY_POINTS))
    for name in ao.ENTRY_POINTS:
        assert re.search(rf'^extern "C" (int|size_t) {name}\(', SRC, re.M), f"{name} is not defined in csrc/augment.hip"
        assert re.search(rf"^(size_t|int) {name}\(", HEADER, re.M), f"{name} is not declared in include/ssv_hip.h"
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    assert set(forms.documented_labels().values()) == set(ao.ENTRY_POINTS), "the docstring table of the GPU file names every entry point"
    assert set(ao.BASES) | {"ssv_augment_workspace_bytes", "ssv_augment_blur_workspace_bytes"} == set(ao.ENTRY_POINTS)


def test_plan_restatement_is_the_sources():
    from ssv_amd import _lib
    assert re.search(rf"^constexpr int NPARAM = {ao.NPARAM};", SRC, re.M) and re.search(rf"^constexpr int KMAX = {ao.KMAX};", SRC, re.M)
    assert re.search(r"^constexpr int PRECISION_BITS = 32 - 8 - 2;", SRC, re.M) and A._PRECISION_BITS == 22
    m = re.search(r"unsigned grid_for\(int64_t n\) \{\s*int64_t b = cdiv64\(n, (\d+)\);\s*if \(b > (\d+)\) b = (\d+);", SRC)
    assert m and [int(g) for g in m.groups()] == [ao.THREADS, ao.GRID_CAP, ao.GRID_CAP]
    assert SRC.count("(int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256") == 2            # aug_views_k and center_view_k stride by the grid
    assert SRC.count("dim3(grid_for(") == 3 and len(re.findall(r"dim3\(grid_for\(\(int64_t\)[^)]*\)\), dim3\(256\)", SRC)) == 3
    for kernel in ("aug_params_k", "aug_blur_params_k"):
        assert f"hipLaunchKernelGGL({kernel}, dim3(cdiv(nviews * B, {ao.PARAM_THREADS})), dim3({ao.PARAM_THREADS})" in SRC
    assert f"hipLaunchKernelGGL(multicrop_params_k, dim3(cdiv(B * ncrop, {ao.PARAM_THREADS})), dim3({ao.PARAM_THREADS})" in SRC
    assert "for (int i = threadIdx.x; i < Ho + Wo; i += 256)" in SRC and "hipLaunchKernelGGL(aug_prep_k, dim3(nviews * B), dim3(256)" in SRC
    # the blur classes: plane2 against the LDS sizes, in this order
    assert "const int plane2 = 2 * ((Ho * Wo + 15) / 16 * 16);" in SRC and "if ((n & 15) == 0) {" in SRC
    got = re.findall(r"(?:if|else if) \(plane2 <= (\d+)\) launch_blur<(\d+), (\d+)>", SRC) + re.findall(r"(else) launch_blur<(\d+), (\d+)>", SRC)
    assert [(int(t), int(l), int(n)) for t, l, n in got[:3]] == [(lds, lds, n) for lds, n in ao.BLUR_CLASSES[:3]]
    assert (int(got[3][1]), int(got[3][2])) == ao.BLUR_CLASSES[3] and len(got) == 4 and ao.BLUR_CLASSES[3][0] == 2 * ao.BLUR_MAX_PIXELS
    # the acceptance rule, the limits, the round-half-to-even offset
    assert SRC.count("SSV_REQUIRE(2 * (Hs + Ho - 1) / Ho + 1 <= KMAX && 2 * (Ws + Wo - 1) / Wo + 1 <= KMAX,") == 2
    assert SRC.count("SSV_REQUIRE((int64_t)Hs * Ws < (1 << 24),") == 2 and ao.MAX_SOURCE_PIXELS == 1 << 24
    assert re.search(rf"^#define SSV_BLUR_MAX_PIXELS {ao.BLUR_MAX_PIXELS}\b", HEADER, re.M) and re.search(r"^#define SSV_BLUR_MAX_SIGMA 1000\.0$", HEADER, re.M)
    assert (_lib.BLUR_MAX_PIXELS, _lib.BLUR_MAX_SIGMA) == (ao.BLUR_MAX_PIXELS, ao.BLUR_MAX_SIGMA)
    assert f"constexpr size_t BLUR_STAGE_ALIGN = {ao.BLUR_STAGE_ALIGN};" in SRC and "constexpr uint32_t BLUR_VIEW_BASE = 1024;" in SRC and bo.BLUR_VIEW_BASE == 1024
    assert "(d % 2 == 0) ? d / 2 : ((d / 2) % 2 == 0 ? d / 2 : d / 2 + 1)" in SRC
    py_round_half = lambda d: d // 2 if d % 2 == 0 else (d // 2 if (d // 2) % 2 == 0 else d // 2 + 1)
    assert all(py_round_half(d) == ao.center_offset(d) for d in range(200))
    assert re.search(r"SSV_OK = 0,\s*SSV_ERR_INVALID = -1,[^\n]*\n\s*SSV_ERR_WORKSPACE = -2,", HEADER) and (ao.OK, ao.ERR_INVALID, ao.ERR_WORKSPACE) == (0, -1, -2)
    assert "3.0 / 4.0, 4.0 / 3.0, seed, step, sample_ids, sample0, boxes);" in SRC                                      # the ratio range of ssv_multicrop_params
    # the workspace sizes are the library's (it loads, and sizes, without a GPU)
    lib = _lib.load()
    shapes = [ao.case_shape(c) for c in ao.PIXEL_CASES if c.entry != "center"] + [(b, v, 0, 0) + o for b in (1, 3, 41) for v in (1, 2, 16)
                                                                                 for o in ((1, 1), (3, 260), (320, 256), (321, 256), (512, 512), (1, 81920), (1, 81921))]
    for b, v, _, _, ho, wo in shapes:
        assert lib.ssv_augment_workspace_bytes(b, v, ho, wo) == ao.workspace_bytes(b, v, ho, wo) > 0
        assert lib.ssv_augment_blur_workspace_bytes(b, v, ho, wo) == ao.blur_workspace_bytes(b, v, ho, wo)
        assert (ao.blur_workspace_bytes(b, v, ho, wo) > 0) == (ho * wo <= ao.BLUR_MAX_PIXELS)
    for shape in ao.WORKSPACE_REFUSALS:
        assert lib.ssv_augment_workspace_bytes(*shape) == 0 == lib.ssv_augment_blur_workspace_bytes(*shape) == ao.workspace_bytes(*shape) == ao.blur_workspace_bytes(*shape)
    for shape in ao.BLUR_WORKSPACE_REFUSALS:
        assert lib.ssv_augment_blur_workspace_bytes(*shape) == 0 == ao.blur_workspace_bytes(*shape) and lib.ssv_augment_workspace_bytes(*shape) > 0
    assert [ao.accepted(s, 32) for s in (96, 97)] == [True, False] and ao.accepted(3 * 37, 37) and not ao.accepted(4 * 37, 37)


def test_case_table_covers_every_documented_branch():
    """the label table of the GPU file is the one its cases name: every documented label has a case and a test, and no case names an undocumented one"""
    import test_gpu_augment_forms as forms
    doc = forms.documented_labels()
    labels = {c.label for c in ao.PIXEL_CASES} | {c["label"] for c in ao.PARAM_CASES + ao.BOX_CASES + ao.REFUSALS}
    assert labels <= set(doc), f"cases name undocumented branches: {sorted(labels - set(doc))}"
    assert set(forms.CASE_LABELS) == {c.id for c in ao.PIXEL_CASES} | {c["id"] for c in ao.PARAM_CASES + ao.BOX_CASES + ao.REFUSALS}
    assert all(forms.CASE_LABELS[c.id] == c.label for c in ao.PIXEL_CASES)
    used = {b for targets in forms.TARGETS.values() for b in targets.split()}
    assert not set(doc) - used, f"documented branches without a test: {sorted(set(doc) - used)}"
    assert not used - set(doc), f"tests name undocumented branches: {sorted(used - set(doc))}"
    assert set(forms.TARGETS) == {name for name in dir(forms) if name.startswith("test_")}
    assert set(doc) - labels == {"front.end", "buffers.guarded", "det.calls"}                    # held by every case, or on the inputs of other labels
    for label, entry in doc.items():
        for c in by_label(label):
            assert {"views": "ssv_augment_views", "blur": "ssv_augment_views_blur", "center": "ssv_center_view"}[c.entry] == entry, c.id
    ids = [c.id for c in ao.PIXEL_CASES] + [c["id"] for c in ao.PARAM_CASES + ao.BOX_CASES + ao.REFUSALS]
    assert len(ids) == len(set(ids))


# ---- the properties the labels claim ----------------------------------------------------------------------------------------------------------------------------------
def _taps(c):
    _, _, _, _, ho, wo = ao.case_shape(c)
    p = c.params.reshape(-1, ao.NPARAM)
    return (max(int(ao.coeffs(int(h), ho)[1].max()) for h in set(p[:, 12])), max(int(ao.coeffs(int(w), wo)[1].max()) for w in set(p[:, 13])))


@pytest.mark.parametrize("case", ao.PIXEL_CASES, ids=lambda c: c.id)
def test_pixel_case_has_the_property_its_label_claims(case):
    ao.check_case(case)
    b, v, hs, ws, ho, wo = ao.case_shape(case)
    pixels, p = v * b * ho * wo, case.params
    stride = case.label in ("views.stride", "center.stride") or case.id == "views.colours"
    assert (ao.trips(pixels) >= 2) == stride and (not stride or pixels > ao.GRID_CAP * ao.THREADS), (pixels, ao.trips(pixels))
    if case.entry != "center":
        ty, tx = _taps(case)
        assert ty <= ao.MAX_TAPS and tx <= ao.MAX_TAPS and (ho + wo > 256 or case.label != "views.tabs")
    if case.label == "views.order":
        assert (p[..., 0] == 1).all() and {tuple(int(x) for x in r[1:5]) for r in p[0]} == set(ao.ORDERS) and len(ao.ORDERS) == 24
        assert {tuple(r[5:9]) for r in p.reshape(-1, 16)} == {tuple(np.float32(f)) for f in ao.FACTOR_SETS} and set(p[..., 9].ravel()) == {0.0, 1.0}
        assert all(sorted(set(p[vi, :, 9])) == [float(vi % 2)] for vi in range(v)) and v == 8
    if case.label == "views.colours":
        assert [ao.hue_shift_of(r) for r in p[:, 0]] == [0, 1, 255, 127, 129] and (p[..., 5:8] == 1).all() and (p[..., 10:14] == [0, 0, 512, 512]).all() and (ho, wo) == (512, 512)
        lat = case.imgs[0].reshape(-1, 3)
        assert len(np.unique(lat, axis=0)) == 64 ** 3 and {0, 1, 2, 253, 254, 255} <= set(np.unique(lat).tolist()) and len(np.unique(lat)) == 64
        assert (case.imgs[1] == 0).all() and (case.imgs[2] == 255).all() and (case.imgs[3][..., 0] == case.imgs[3][..., 2]).all() and len(np.unique(case.imgs[3])) > 100
    if case.label == "views.crop":
        boxes = {tuple(int(x) for x in r[10:14]) for r in p.reshape(-1, 16)}
        assert boxes == set(ao.CROP_BOXES) and (hs, ws) == (24, 30)
        assert {(0, 0, 1, 1), (0, ws - 1, 1, 1), (hs - 1, 0, 1, 1), (hs - 1, ws - 1, 1, 1), (0, 0, hs, ws)} <= boxes
        assert any(h == 1 and w == ws for _, _, h, w in boxes) and any(h == hs and w == 1 for _, _, h, w in boxes) and (3, 4, 2, 3) in boxes
        assert any(t + h == hs and l + w == ws and (h, w) == (8, 10) for t, l, h, w in boxes)
        if (ho, wo) == (8, 10):                                           # x3 on both axes, on one axis only, and identity coefficients
            assert _taps(case) == (6, 6) and {(24, 30), (24, 10), (8, 30), (8, 10)} <= {(h, w) for _, _, h, w in boxes}
            assert int(ao.coeffs(24, 8)[1].max()) == 6 == ao.MAX_TAPS and (ao.coeffs(10, 10)[2][:, 0] == 1 << 22).all() and (ao.coeffs(10, 10)[2][:, 1:] == 0).all()
            assert ((ao.coeffs(23, 8)[2] > 0).sum(1) == 6).any() and ((ao.coeffs(29, 10)[2] > 0).sum(1) == 6).any() and (1, 1, 23, 29) in boxes
            assert not ao.accepted(25, 8) and not ao.accepted(31, 10)     # six taps are the most the rule lets through (test_the_acceptance_rule_lets_six_taps_through): one more source row is refused
        else:
            assert (ho, wo) == (32, 32) and _taps(case) <= (3, 3)
    if case.label == "views.out":
        assert (p[0, :, 14] == 1).all() and (p[1, :, 14] == 0).all() and (ho != wo or (ho, wo) == (1, 1)) and (wo % 2 == 1) and (v * b * ho * wo) % 256 != 0
    if case.label == "views.tabs":
        assert (ho, wo) == (3, 260) and ho + wo > 256
    if case.label == "views.mean":
        assert (p[..., 0] == 1).all() and (hs * ws < 256 or (hs, ws) == (17, 19))
        if (hs, ws) == (1, 2):                                            # the luma mean in front of the contrast op is exactly k + 0.5
            for vi in range(v):
                for k in range(b):
                    l = ao.prefix_luma(case.imgs[k], p[vi, k])
                    assert Fraction(int(l.sum()), l.size).denominator == 2, (vi, k)
            assert {tuple(int(x) for x in r[1:5]).index(1) for r in p.reshape(-1, 16)} == {0, 1}
    if case.label == "views.stride":
        assert (b, v, ho, wo) == (41, 2, 160, 160) and pixels == 2099200 and len(ao.distinct_views(case)) == 8
    if case.label == "views.ids":
        assert {ao.case_shape(c)[1] for c in by_label("views.ids")} == {1, 2, 5} and {c.ids is None for c in by_label("views.ids")} == {True, False}
        assert case.ids is None or (len(set(case.ids.tolist())) < len(case.ids) and case.ids.tolist() != sorted(case.ids.tolist()))
    if case.label == "blur.class":
        want = dict(zip(ao.BLUR_CLASS_OUTS, ((1, True), (1, False), (2, True), (2, True), (3, True), (3, False), (4, False), (4, True))))
        cls, lds, threads, vector = ao.blur_class(ho, wo)
        assert (cls, vector) == want[(ho, wo)] and (b, v) == (2, 2) and sorted(p[..., 15].ravel().tolist()) == [0.0, np.float32(0.3), 2.0, 8.0]
        assert 2 * ((ho * wo + 15) // 16 * 16) <= lds and (lds, threads) == ao.BLUR_CLASSES[cls - 1]
        assert (ho, wo) != (128, 128) or 2 * ho * wo == 32768
        assert (ho, wo) != (181, 181) or (ho * wo < 32768 == (ho * wo + 15) // 16 * 16)
        assert (ho, wo) != (320, 256) or ho * wo == ao.BLUR_MAX_PIXELS
    if case.label == "blur.thin":
        assert min(ho, wo) == 1 and (p[..., 15] > 0).sum() == 3
    if case.label == "blur.mixed":
        assert bool((p[..., 15] > 0).all()) == case.id.endswith("all") and bool((p[..., 15] == 0).all()) == case.id.endswith("none")
    if case.label == "center.round":
        assert (hs - ho) in ao.ROUND_DIFFS and (ws - wo) in ao.ROUND_DIFFS
    if case.label == "center.stride":
        assert (b, ho, wo) == (33, 256, 256) and pixels == 2162688 and len(case.imgs) == 3 and (hs - ho, ws - wo) == (1, 3)


def test_tables_hold_every_case_of_their_labels():
    assert {ao.case_shape(c)[4:] for c in by_label("blur.class")} == set(ao.BLUR_CLASS_OUTS) and len(by_label("blur.class")) == 8
    assert {(ao.case_shape(c)[2] - 4, ao.case_shape(c)[3] - 5) for c in by_label("center.round")} == {(a, b) for a in ao.ROUND_DIFFS for b in ao.ROUND_DIFFS}
    assert {ao.center_offset(d) - d // 2 for d in ao.ROUND_DIFFS if d % 2 and (d // 2) % 2 == 0} == {0} and {ao.center_offset(d) - d // 2 for d in (3, 7)} == {1}
    assert {ao.case_shape(c)[4:] for c in by_label("blur.thin")} == {(1, 40), (40, 1)} and {ao.case_shape(c)[2:4] for c in by_label("views.mean")} == {(1, 2), (5, 7), (17, 19)}
    tails = {(pc["B"], pc["V"]) for pc in ao.PARAM_CASES if pc["label"] == "params.tail"}
    assert tails == {(1, 1), (63, 1), (32, 2), (65, 1), (13, 5), (9, 16)} == {(pc["B"], pc["V"]) for pc in ao.PARAM_CASES if pc["label"] == "params.blur" and pc["blur"] == (0.5, 0.1, 2.0)}
    assert sorted(b * v % ao.PARAM_THREADS for b, v in tails) == [0, 1, 1, 1, 16, 63] and max(v for _, v in tails) == 16
    assert {pc["blur"][0] for pc in ao.PARAM_CASES if pc["blur"]} == {0.0, 0.5, 1.0} and any(pc["blur"] and pc["blur"][1] == pc["blur"][2] for pc in ao.PARAM_CASES)
    assert sorted(bc["B"] * bc["ncrop"] for bc in ao.BOX_CASES if bc["label"] == "boxes.tail") == [1, 63, 64, 65]
    assert {bc["view_base"] for bc in ao.BOX_CASES} == {16, 144, 400, 65535} and all(bc["view_base"] + bc["ncrop"] <= 65536 and bc["view_base"] >= 16 for bc in ao.BOX_CASES)
    cfgs = {pc["id"]: pc["cfg"] for pc in ao.PARAM_CASES if pc["label"] == "params.cfg"}
    assert len(cfgs) == 6 and cfgs["params.cfg-bright"]["brightness"] == 1.5 and cfgs["params.cfg-scale"]["scale_min"] == cfgs["params.cfg-scale"]["scale_max"]
    assert cfgs["params.cfg-ratio"]["ratio_min"] == cfgs["params.cfg-ratio"]["ratio_max"] == 1.0
    for pc in ao.PARAM_CASES:
        assert ao.verdict("ssv_augment_params_blur" if pc["blur"] else "ssv_augment_params",
                          dict(B=pc["B"], Hs=pc["hs"], Ws=pc["ws"], nviews=pc["V"], cfg=pc["cfg"], params=True, p_blur=(pc["blur"] or [0])[0],
                               sigma_min=(pc["blur"] or [0, 0])[1], sigma_max=(pc["blur"] or [0, 0, 0])[2])) == ao.OK, pc["id"]
    for bc in ao.BOX_CASES:
        assert ao.verdict("ssv_multicrop_params", dict(B=bc["B"], Hs=bc["hs"], Ws=bc["ws"], ncrop=bc["ncrop"], view_base=bc["view_base"], boxes=True,
                                                       scale_min=bc["scale"][0], scale_max=bc["scale"][1])) == ao.OK, bc["id"]


# ---- Pillow is the authority ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ao.PIXEL_CASES, ids=lambda c: c.id)
def test_pillow_agrees_with_the_restatement_on_every_pixel_case(case):
    """view_numpy == view_pil, view_numpy_blur == view_pil_blur, the centre view == center_view_pil, and the restatement the GPU file compares against (the
    kernels' walk: both passes always, NHWC) equals all of them, bit for bit, on every distinct (image, record) of the case"""
    ref = ao.reference(case)
    b, v = ao.case_shape(case)[:2]
    assert ref.dtype == np.float32 and ref.shape == ((b,) if case.entry == "center" else (v, b)) + tuple(case.out_hw) + (3,) and np.isfinite(ref).all()
    for (i, _), (img, p) in ao.distinct_views(case).items():
        if case.entry == "center":
            mine, old, pil = ao.center_view(img, case.out_hw), A.center_view_pil(img, case.out_hw, ao.MEAN, ao.STD), A.center_view_pil(img, case.out_hw, ao.MEAN, ao.STD)
        elif case.entry == "views":
            mine, old, pil = ao.view(img, p, case.out_hw), A.view_numpy(img, p, case.out_hw, ao.MEAN, ao.STD), A.view_pil(img, p, case.out_hw, ao.MEAN, ao.STD)
            assert p[15] == 0
        else:
            mine, old = ao.view(img, p, case.out_hw, blur=True), bo.view_numpy_blur(img, p, case.out_hw, ao.MEAN, ao.STD)
            pil = bo.view_pil_blur(img, p, case.out_hw, ao.MEAN, ao.STD)
        np.testing.assert_array_equal(_bits(old), _bits(pil), err_msg=f"{case.id}: the restatement differs from Pillow on image {i}, record {p}")
        np.testing.assert_array_equal(_bits(mine.transpose(2, 0, 1)), _bits(pil), err_msg=f"{case.id}: the kernels' walk differs from Pillow on image {i}, record {p}")


def test_centre_offset_is_pillows_crop():
    """the offset rule itself against PIL.Image.crop at the box torchvision's center_crop computes"""
    from PIL import Image
    for c in by_label("center.round"):
        for img in c.imgs:
            h, w = img.shape[:2]
            top, left = int(round((h - c.out_hw[0]) / 2.0)), int(round((w - c.out_hw[1]) / 2.0))
            crop = np.asarray(Image.fromarray(img, "RGB").crop((left, top, left + c.out_hw[1], top + c.out_hw[0])), dtype=np.uint8)
            np.testing.assert_array_equal(_bits(ao.normalise(crop)), _bits(ao.center_view(img, c.out_hw)))


# ---- conditions on the inputs ---------------------------------------------------------------------------------------------------------------------------------------------
def test_draw_restatement_is_the_older_one_and_the_counter_holds_48_bits():
    for sample, view, hw in ((0, 0, (40, 36)), (17, 1, (32, 32)), (1000, 15, (8, 64)), ((1 << 32) + 5, 3, (30, 40))):
        np.testing.assert_array_equal(ao.draw_record(ao.SEED, ao.STEP, sample, view, *hw)[0], A.draw_params(ao.SEED, ao.STEP, sample, view, *hw))
        old = {"apply_prob": 0.3, "gray_prob": 0.6, "flip_prob": 0.1, "scale": (0.5, 0.7), "ratio": (0.9, 1.1), "brightness": 1.5, "hue": 0.3}
        new = dict(p_jitter=0.3, p_gray=0.6, p_flip=0.1, scale_min=0.5, scale_max=0.7, ratio_min=0.9, ratio_max=1.1, brightness=1.5, hue=0.3)
        np.testing.assert_array_equal(ao.draw_record(ao.SEED, ao.STEP, sample, view, *hw, cfg=new)[0], A.draw_params(ao.SEED, ao.STEP, sample, view, *hw, cfg=old))
        got = ao.draw_record(ao.SEED, ao.STEP, sample, view, *hw, blur=(0.5, 0.1, 2.0))[0]
        assert got[15] == bo.draw_blur(ao.SEED, ao.STEP, sample, view, 0.5, 0.1, 2.0) and (got[:15] == A.draw_params(ao.SEED, ao.STEP, sample, view, *hw)[:15]).all()
    rec = lambda **kw: ao.draw_record(**dict(dict(seed=ao.SEED, step=ao.STEP, sample=5, view=0, hs=40, ws=36), **kw))[0]
    assert (rec(sample=(1 << 48) + 5) == rec()).all() and not (rec(sample=(1 << 32) + 5) == rec()).all()
    assert (rec(step=(1 << 32) + 7) == rec()).all() and not (rec(seed=(0xDEADBEEF << 32) | 420) == rec()).all() and not (rec(view=1) == rec()).all()
    big = next(pc for pc in ao.PARAM_CASES if pc["id"] == "params.ids-big")
    r = ao.param_records(big)[0]
    assert (r[:, 1] == r[:, 2]).all() and not (r[:, 0] == r[:, 1]).all()
    # a box of ssv_multicrop_params is the crop draw alone on its own stream
    box, branch, _ = ao.draw_boxes(ao.SEED, ao.STEP, 3, 16, 1, 32, 32, (0.3, 1.0))
    assert (box, branch) == ao.sample_rrc(A._Stream(ao.SEED, ao.STEP, 3, 17), 32, 32, 0.3, 1.0, 0.75, 4.0 / 3.0)[:2] and branch == "accept"


def test_crop_draws_take_every_branch():
    """each of the four branches of sample_rrc by at least 8 records of its case; the fallback boxes are the ones worked by hand"""
    for table, records in ((ao.PARAM_CASES, ao.param_records), (ao.BOX_CASES, ao.box_records)):
        rrc = [c for c in table if c["label"].endswith(".rrc")]
        assert [(c["hs"], c["ws"]) for c in rrc] == [hw for hw, _, _ in ao.RRC_SOURCES]
        for c, (hw, scale, want) in zip(rrc, ao.RRC_SOURCES):
            recs, branches, _ = records(c)
            flat = [x for row in branches for x in row]
            count = {k: flat.count(k) for k in ("accept", "wide", "tall", "whole")}
            print(c["id"], count)
            boxes = (recs[..., 10:14] if recs.shape[-1] == 16 else recs).reshape(-1, 4).astype(np.int64)
            if want == "whole":
                assert count["whole"] >= 8 and count["accept"] >= 8 and count["wide"] == count["tall"] == 0
                assert count["whole"] + count["accept"] == len(flat) and (count["whole"] == 106 or "boxes" in c["id"])      # an attempt is accepted iff the ratio exceeds 1.29: 5.7 % of them
                assert all((bx == (0, 0) + hw).all() for bx, br in zip(boxes, flat) if br == "whole")
            else:
                assert count[want] == len(flat) >= 8
                assert (boxes == {"wide": (0, 26, 8, 11), "tall": (26, 0, 11, 8)}[want]).all()
    plain = [x for pc in ao.PARAM_CASES if pc["label"] == "params.tail" for row in ao.param_records(pc)[1] for x in row]
    assert plain.count("accept") >= 8


@pytest.mark.parametrize("case", ao.PARAM_CASES + ao.BOX_CASES, ids=lambda c: c["id"])
def test_no_draw_lies_near_a_decision_boundary(case):
    """sqrt(..) + 0.5 and u (n + 1) against an integer, every probability draw against its threshold: all farther than 1e-9, four orders of magnitude above what an
    ulp or two of the device's log / exp / sqrt could move; and every drawn box lies inside its source"""
    recs, _, margin = (ao.param_records if "V" in case else ao.box_records)(case)
    print(case["id"], f"smallest margin {margin:.3g}")
    assert margin > ao.MARGIN == 1e-9
    boxes = (recs[..., 10:14] if recs.shape[-1] == 16 else recs).reshape(-1, 4).astype(np.int64)
    assert (boxes[:, :2] >= 0).all() and (boxes[:, 2:] >= 1).all() and (boxes[:, 0] + boxes[:, 2] <= case["hs"]).all() and (boxes[:, 1] + boxes[:, 3] <= case["ws"]).all()
    if "V" in case:
        assert (np.sort(recs[..., 1:5], -1) == np.arange(4)).all()
        c = case["cfg"]
        if case["id"] == "params.cfg-zero":
            assert (recs[..., 5:8] == 1).all() and (recs[..., 8] == 0).all()
        if case["id"] in ("params.cfg-p0", "params.cfg-p1"):
            assert (recs[..., [0, 9, 14]] == c["p_jitter"]).all()
        if case["id"] == "params.cfg-bright":
            assert recs[..., 5].min() < 0.5 and recs[..., 5].max() > 2.0 and recs[..., 5].min() >= 0.0
        if case["id"] == "params.cfg-ratio":
            assert (np.abs(recs[..., 12] - recs[..., 13]) <= 0).all()
        if case["blur"]:
            on = recs[..., 15] > 0
            assert {0.0: not on.any(), 1.0: on.all()}.get(case["blur"][0], on.any() and not on.all() or recs[..., 15].size < 8)
            assert case["blur"][1] != case["blur"][2] or set(recs[..., 15][on].tolist()) == {case["blur"][1]}


def test_colour_cases_reach_every_branch_of_the_hsv_round_trip_and_both_clip_ends():
    case = ao.PIXEL_BY_ID["views.colours"]
    lat = case.imgs[0].astype(np.int64)
    r, g, b = lat[..., 0], lat[..., 1], lat[..., 2]
    maxc, minc = lat.max(-1), lat.min(-1)
    live = maxc != minc
    assert (live & (r == maxc)).any() and (live & (r != maxc) & (g == maxc)).any() and (live & (r != maxc) & (g != maxc)).any() and (~live).any()
    hsv = A._rgb2hsv(case.imgs[0])
    assert (hsv[..., 1] == 0).any() and (hsv[..., 1][live] > 0).all() and {0, 255} <= set(np.unique(hsv[..., 2]).tolist())
    stats = {}
    for vi in range(len(ao.HUE_FACTORS)):
        ao.view(case.imgs[0], case.params[vi, 0], case.out_hw, stats=stats)
        assert stats["sectors"] == set(range(6)), (vi, stats["sectors"])
        stats.clear()
    stats = {}
    ao.reference(ao.PIXEL_BY_ID["views.order"], stats=stats)
    assert stats["low"] > 0 and stats["high"] > 0, stats


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", ao.REFUSALS, ids=lambda r: r["id"])
def test_refusal_is_decided_before_anything_is_launched(r):
    """the restated SSV_REQUIREs accept the unchanged call and give the changed one its code - and so does the library itself, called here without a GPU on
    addresses it must never read: a refused call returns before its first launch"""
    from ssv_amd import _lib
    base, changed = ao.call_of(r)
    assert ao.verdict(r["entry"], base) == ao.OK and ao.verdict(r["entry"], changed) == r["rc"] != ao.OK
    assert sum(base[k] != changed[k] and not (base[k] != base[k] and changed[k] != changed[k]) for k in base) == 1, "one changed argument"
    lib = _lib.load()
    three = (C.c_float * 3)(0.5, 0.5, 0.5)
    sizer = {"ssv_augment_views": ao.workspace_bytes, "ssv_augment_views_blur": ao.blur_workspace_bytes}.get(r["entry"])
    need = sizer(*(changed[k] for k in ("B", "nviews", "Ho", "Wo"))) if sizer else 0
    ptr = lambda name: need if name == "ws_bytes" else (C.addressof(three) if name in ("mean", "std") else 4096)      # 4096: a page nothing maps
    rc = getattr(lib, r["entry"])(*ao.marshal(r["entry"], changed, ptr, None))
    assert rc == r["rc"], (rc, lib.ssv_last_error().decode())
    msg = lib.ssv_last_error().decode()
    inner = "ssv_augment_params" if r["entry"] == "ssv_augment_params_blur" and isinstance(r["change"].get("cfg"), dict) else r["entry"]      # the crop ranges are refused by the entry point the blur one calls
    assert msg.startswith(inner + ":"), msg


def test_refusals_cover_every_require():
    """every SSV_REQUIRE / SSV_FAIL of the eight entry points is the first to fail for at least one refusal (by its message)"""
    from ssv_amd import _lib
    lib = _lib.load()
    seen = set()
    three = (C.c_float * 3)(0.5, 0.5, 0.5)
    for r in ao.REFUSALS:
        _, changed = ao.call_of(r)
        sizer = {"ssv_augment_views": ao.workspace_bytes, "ssv_augment_views_blur": ao.blur_workspace_bytes}.get(r["entry"])
        need = sizer(*(changed[k] for k in ("B", "nviews", "Ho", "Wo"))) if sizer else 0
        ptr = lambda name: need if name == "ws_bytes" else (C.addressof(three) if name in ("mean", "std") else 4096)
        assert getattr(lib, r["entry"])(*ao.marshal(r["entry"], changed, ptr, None)) == r["rc"]
        seen.add(re.sub(r"[\d.]+", "#", lib.ssv_last_error().decode())[:60])
    body = SRC[SRC.index('extern "C" int ssv_augment_params('):]
    want = 0
    for name in ao.ENTRY_POINTS:
        part = body[body.index(f" {name}("):]
        part = part[:part.index("\n}\n")]
        want += len(re.findall(r"SSV_REQUIRE\(|SSV_FAIL\(SSV_ERR_WORKSPACE", part))
    print(sorted(seen))
    assert len(seen) == want == 19, (len(seen), want)


def test_the_acceptance_rule_lets_six_taps_through():
    """2 (src + out - 1) / out + 1 <= KMAX means src <= 3 out: the triangle filter's support is at most 3 source pixels to either side, which covers at most six pixel
    centres.  So no accepted shape has a seventh tap, KMAX = 8 is never the binding cap, and a kernel that capped the count at 6 (the mutant `taps6`) computes the
    same bits at every accepted shape: that mistake cannot be observed through the ABI.  A cap of 5 (`taps5`) can, and the cases notice it."""
    most = 0
    for out in range(1, 41):
        for src in range(1, 4 * out + 2):
            if ao.accepted(src, out):
                assert src <= 3 * out
                xmin, count, kk = ao.coeffs(src, out)
                most = max(most, int(count.max()))
                assert (kk[:, 6:] == 0).all() and all((a == b).all() for a, b in zip(ao.coeffs(src, out, 6), (xmin, count, kk[:, :6])))
            else:
                assert src > 3 * out
    assert most == 6 == ao.MAX_TAPS and ao.UNOBSERVABLE == {"taps6"}
    for c in by_label(ao.MUTANTS["taps6"]):
        np.testing.assert_array_equal(_bits(ao.reference(c, mutant="taps6")), _bits(ao.reference(c)))


# ---- sensitivity ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", sorted(set(ao.MUTANTS) - ao.UNOBSERVABLE))
def test_cases_notice_each_deliberate_mistake(mutant):
    label = ao.MUTANTS[mutant]
    cases = by_label(label)
    assert cases and label in {c.label for c in ao.PIXEL_CASES}
    changed = {c.id: int((_bits(ao.reference(c, mutant=mutant)) != _bits(ao.reference(c))).sum()) for c in cases}
    print(mutant, {k: v for k, v in changed.items() if v})
    assert any(changed.values()), f"no case of {label} would notice {mutant}"
    if mutant == "center_half_up":                                         # ... and plain truncation: the floor is odd at 3 and 7
        trunc = [c.id for c in cases if any((d % 2) and d // 2 != ao.center_offset(d) for d in (c.imgs.shape[1] - 4, c.imgs.shape[2] - 5))]
        assert len(trunc) == 20 and sum(v > 0 for v in changed.values()) == 11


# ---- the committed report --------------------------------------------------------------------------------------------------------------------------------------------
def test_the_committed_report_holds_every_case_with_no_mismatch():
    """profiles/augment_forms_report.json (an MI355X run of tests/test_gpu_augment_forms.py): every case of the tables and the front-end pass, its label and shape,
    the elements compared, zero mismatches and the measured wall seconds"""
    import json
    import test_gpu_augment_forms as forms
    doc = json.load(open(os.path.join(ROOT, "profiles", "augment_forms_report.json")))
    assert re.fullmatch(r"[0-9a-f]{16}", doc["source_sha16"]) and set(doc) == {"source_sha16", "cases"}
    assert set(doc["cases"]) == set(forms.CASE_LABELS) | {"front.end"}
    for cid, r in doc["cases"].items():
        assert set(r) == {"label", "shape", "elements", "mismatches", "seconds"} and r["mismatches"] == 0 and r["elements"] > 0 and r["seconds"] >= 0, cid
        assert r["label"] == forms.CASE_LABELS.get(cid, "front.end")
    for c in ao.PIXEL_CASES:
        b, v, _, _, ho, wo = ao.case_shape(c)
        assert doc["cases"][c.id]["shape"] == list(ao.case_shape(c)) and doc["cases"][c.id]["elements"] == v * b * ho * wo * 3
    assert {r["label"] for r in doc["cases"].values()} == set(forms.documented_labels()) - {"buffers.guarded", "det.calls"}
