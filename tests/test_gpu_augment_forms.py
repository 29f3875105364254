"""GPU: every entry point of csrc/augment.hip at the shapes where its launch decisions flip - straight through the C ABI on guarded buffers - against the numpy
restatements of tests/augment_forms_oracle.py, bit for bit: everything up to the final ToTensor / Normalize is integer arithmetic, and those three float32
operations are IEEE ones, so every comparison is `assert_array_equal` on bits, nothing is excused and there is no tolerance.  tests/test_augment_forms_cpu.py
proves without a GPU that Pillow agrees with the restatement on every pixel case below, that every case has the property its label names, that no draw lies within
1e-9 of a decision boundary, and that the cases would notice eight deliberate mistakes (and that a ninth, a tap count capped at 6, cannot be observed at any accepted shape).  This file imports no Pillow.

Held for every case: outputs are views into NaN-prefilled buffers (integer outputs: -5) with 1024 guard elements behind them; workspaces are sized by the
library's own *_workspace_bytes, filled with a byte pattern and guarded; no output element keeps its prefill, every guard is untouched, every input is
bit-identical afterwards, and a second identical call gives the same bits.  No record ever names a crop box outside its source or an order slot outside 0..3
(augment_forms_oracle.check_case runs in front of every launch): the library cannot validate device-resident records.

Branch labels (label, entry point, what the cases reach; the shapes are in tests/augment_forms_oracle.py):

  params.tail          ssv_augment_params       (B, V) = (1, 1) (63, 1) (32, 2) (65, 1) (13, 5) (9, 16): the edges of the 64-thread blocks; view keys 0..15, each its own stream
  params.ids           ssv_augment_params       null ids with sample0 = 1000 against explicit ids; ids 2^32 + 5 and 2^48 + 5 (the counter holds 48 bits); step 2^32 + 7; a seed with a high half
  params.rrc           ssv_augment_params       sources 8 x 64, 64 x 8 (scale 0.9 .. 1) and 30 x 40 (scale 1): the wide, tall and whole fallbacks of sample_rrc, and accept
  params.cfg           ssv_augment_params       every strength 0; probabilities 0 and 1; brightness 1.5 (the lower bound clamps at 0); scale_min == scale_max; ratio_min == ratio_max == 1
  params.blur          ssv_augment_params_blur  the same tails; p_blur 0, 0.5, 1; sigma_min == sigma_max; slots 0..14 bit-equal to the plain entry point, slot 15 to blur_oracle.draw_blur
  boxes.tail           ssv_multicrop_params     B * ncrop in {1, 63, 64, 65}
  boxes.base           ssv_multicrop_params     view_base 144, 400, and 65535 with one crop
  boxes.rrc            ssv_multicrop_params     the fallback sources
  boxes.ids            ssv_multicrop_params     null ids with sample0 against explicit ids; ids above 2^32
  views.order          ssv_augment_views        all 24 op orders x factor sets (1.8, 1.8, 1.8, 0.5) (0, 0, 0, -0.5) and two inside [0, 1] x grey off / on, 21 x 18 source: the contrast mean behind every prefix, both clip ends of blend1
  views.colours        ssv_augment_views        512 x 512 holding every colour of a 64-level lattice (0, 1, 2, 253, 254, 255 among the levels), all-0, all-255, grey; hue shifts 0, +1, -1, +-0.5: every branch of rgb2hsv / hsv2rgb
  views.crop           ssv_augment_views        whole image; 1 x 1 boxes at the four corners; 1 x Ws, Hs x 1, 2 x 3; up-scaling to 32 x 32; crop == output (identity coefficients); x3 down on both axes and on one: 6 taps, the most the acceptance rule lets through
  views.out            ssv_augment_views        Ho != Wo, odd Wo with flip, Wo = 1 with flip, 1 x 1; pixel counts no multiple of 256
  views.tabs           ssv_augment_views        output 3 x 260: Ho + Wo > 256, the coefficient-table loop of aug_prep_k takes a second trip
  views.mean           ssv_augment_views        sources 1 x 2 whose luma mean is k + 0.5 exactly, 5 x 7 (fewer pixels than threads), 17 x 19
  views.stride         ssv_augment_views        V 2, B 41, 160 x 160: 2 099 200 pixels, the second trip of the grid-stride loop of aug_views_k
  views.ids            ssv_augment_views        null ids equal arange; permuted and repeated ids; V of 1, 2, 5
  blur.class           ssv_augment_views_blur   64 x 64, 65 x 63, 64 x 65, 128 x 128, 128 x 129, 181 x 181, 182 x 181, 320 x 256: the four LDS classes at their edges, vector and scalar fill; sigmas 0.3, 2, 8 and one unblurred record
  blur.thin            ssv_augment_views_blur   outputs 1 x 40 and 40 x 1
  blur.mixed           ssv_augment_views_blur   all records blurred; none blurred: the bits of ssv_augment_views on the same records
  center.round         ssv_center_view          (Hs - Ho, Ws - Wo) over {0, 1, 2, 3, 6, 7} squared: round-half-to-even offsets, the floor even and odd
  center.stride        ssv_center_view          B 33, 256 x 256 from three 257 x 259 images via ids: 2 162 688 pixels, the second trip of center_view_k
  center.ids           ssv_center_view          null ids equal arange; repeated ids
  refuse.params        ssv_augment_params_blur  every SSV_REQUIRE of both draw entry points: sizes 0 and -1, nviews 17, null cfg / params, bad scale and ratio ranges, p_blur -0.1 / 1.1 / NaN, bad sigma ranges
  refuse.views         ssv_augment_views        sizes 0 and -1, null pointers, Hs = 97 against Ho = 32 (96 is accepted), a 4096 x 4096 source (allocated)
  refuse.blur          ssv_augment_views_blur   the same, and outputs of 81921 pixels, 2^30 samples, a workspace 4 bytes off its alignment
  refuse.center        ssv_center_view          sizes 0 and -1, Ho > Hs, Wo > Ws, null pointers
  refuse.boxes         ssv_multicrop_params     sizes 0 and -1, view_base 15, view_base + ncrop = 65537, null boxes, bad scale ranges
  refuse.workspace     ssv_augment_workspace_bytes       a workspace one byte short and of 0 bytes: SSV_ERR_WORKSPACE; sizes the size functions answer with 0
  buffers.guarded      ssv_augment_blur_workspace_bytes  every case: guards, prefills, inputs, workspaces of exactly the library's own size
  det.calls            ssv_augment_views        every case: equal bits between two calls
  front.end            ssv_augment_views        GpuTransform.draw / apply / one_view and MultiCrop.__call__ on the views.crop inputs, each optional transform dropped in turn

Under SSV_AUGMENT_FORMS_REPORT=<path> the file writes profiles/augment_forms_report.json: per case the label, the shape, the elements compared, the mismatches (a
hard zero) and the wall seconds of the two guarded calls and their comparison.
"""
import ctypes as C
import json
import os
import re
import time

import numpy as np
import pytest
import torch

import augment_forms_oracle as ao
import blur_oracle as bo
import forms_report as fr

pytestmark = pytest.mark.gpu
PATTERN = 0x5A                                                           # the byte every workspace is filled with
BOX_UNWRITTEN = -5                                                       # a box entry is >= 0
CASE_LABELS = {**{c.id: c.label for c in ao.PIXEL_CASES}, **{c["id"]: c["label"] for c in ao.PARAM_CASES + ao.BOX_CASES + ao.REFUSALS}}
TARGETS = {"test_param_draws_equal_the_restatement": "params.tail params.ids params.rrc params.cfg params.blur",
           "test_boxes_equal_the_restated_draw": "boxes.tail boxes.base boxes.rrc boxes.ids",
           "test_pixels_bit_for_bit": " ".join(sorted({c.label for c in ao.PIXEL_CASES})) + " buffers.guarded det.calls",
           "test_refusals_touch_nothing": "refuse.params refuse.views refuse.blur refuse.center refuse.boxes refuse.workspace",
           "test_size_functions_answer_refused_shapes_with_zero": "refuse.workspace",
           "test_front_end_pass": "front.end"}
REPORT = {}


def documented_labels():
    out = {}
    for line in __doc__.splitlines():
        m = re.match(r"^  ([a-z0-9_]+\.[a-z0-9_]+)\s+(ssv_\w+)\s+\S", line)
        if m:
            out[m.group(1)] = m.group(2)
    return out


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from ssv_amd import _lib
    yield _lib.load()
    path = os.environ.get("SSV_AUGMENT_FORMS_REPORT")
    if path and REPORT:
        doc = {"cases": {}}
        if os.path.exists(path):
            with open(path) as fh:
                doc = json.load(fh)
        doc["source_sha16"] = _lib.source_sha16()
        doc["cases"].update(REPORT)
        with open(path, "w") as fh:
            json.dump(doc, fh, indent=1, sort_keys=True)


def _note(cid, shape, got, want, t0):
    """record the figures of a case, then hold the hard zero"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (cid, got.shape, want.shape)
    g, w = (got.view(np.int32), want.view(np.int32)) if got.dtype == np.float32 else (got, want)
    bad = int((g != w).sum())
    REPORT[cid] = {"label": CASE_LABELS[cid], "shape": list(shape), "elements": int(want.size), "mismatches": bad, "seconds": round(time.perf_counter() - t0, 4)}
    print(f"{cid}: {bad} of {want.size} elements differ")
    np.testing.assert_array_equal(g, w, err_msg=f"{cid}: first differing elements at {np.argwhere(g != w)[:4].tolist()}")


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def _workspace(nbytes):
    return torch.full((int(nbytes) + fr.GUARD,), PATTERN, dtype=torch.uint8, device="cuda")


def _cfg(c):
    from ssv_amd import _lib
    return _lib.AugCfg(*[float(c[k]) for k in ao.CFG_FIELDS])


# ---- parameter draws --------------------------------------------------------------------------------------------------------------------------------------------------
def _draw(pc, what, blur="case", ids="case"):
    from ssv_amd import _lib
    b, v = pc["B"], pc["V"]
    blur = pc["blur"] if blur == "case" else blur
    ids = pc["ids"] if ids == "case" else ids
    buf = fr.Buffers()
    d_ids = None if ids is None else buf.up("ids", np.asarray(ids, np.int64))
    out = buf.out("params", v * b * ao.NPARAM, torch.float32, float("nan"))
    cfg = _cfg(pc["cfg"])
    sample0 = pc["sample0"] if ids is None else -12345                    # not read when ids are given
    if blur is None:
        _lib.call("ssv_augment_params", b, pc["hs"], pc["ws"], v, C.byref(cfg), pc["seed"], pc["step"], _lib.ptr(d_ids), sample0, _lib.ptr(out), _lib.stream())
    else:
        _lib.call("ssv_augment_params_blur", b, pc["hs"], pc["ws"], v, C.byref(cfg), pc["seed"], pc["step"], _lib.ptr(d_ids), sample0, blur[0], blur[1], blur[2],
                  _lib.ptr(out), _lib.stream())
    buf.verify(what)
    got = out.cpu().numpy().reshape(v, b, ao.NPARAM)
    assert not np.isnan(got).any(), f"{what}: a slot was not written"
    return got


@pytest.mark.parametrize("pc", ao.PARAM_CASES, ids=lambda c: c["id"])
def test_param_draws_equal_the_restatement(lib, pc):
    want, _, margin = ao.param_records(pc)
    assert margin > ao.MARGIN
    t0 = time.perf_counter()
    got = _draw(pc, pc["id"])
    again = _draw(pc, pc["id"] + " (second call)")
    _note(pc["id"], (pc["B"], pc["V"], pc["hs"], pc["ws"]), got, want, t0)
    np.testing.assert_array_equal(got.view(np.int32), again.view(np.int32))
    if pc["blur"] is not None:                                            # slots 0..14 are the plain entry point's, slot 15 the older restatement's
        plain = _draw(pc, pc["id"] + " (plain)", blur=None)
        np.testing.assert_array_equal(got[..., :15].view(np.int32), plain[..., :15].view(np.int32))
        assert (plain[..., 15] == 0).all()
        ids = pc["ids"] if pc["ids"] is not None else [pc["sample0"] + k for k in range(pc["B"])]
        want15 = np.array([[bo.draw_blur(pc["seed"], pc["step"], i, v, *pc["blur"]) for i in ids] for v in range(pc["V"])], np.float32)
        np.testing.assert_array_equal(got[..., 15].view(np.int32), want15.view(np.int32))
    if pc["ids"] is None:                                                 # null ids with sample0 are sample0 + arange
        explicit = _draw(pc, pc["id"] + " (explicit ids)", ids=[pc["sample0"] + k for k in range(pc["B"])])
        np.testing.assert_array_equal(got.view(np.int32), explicit.view(np.int32))


def _boxes(bc, what, ids="case"):
    from ssv_amd import _lib
    ids = bc["ids"] if ids == "case" else ids
    buf = fr.Buffers()
    d_ids = None if ids is None else buf.up("ids", np.asarray(ids, np.int64))
    out = buf.out("boxes", bc["B"] * bc["ncrop"] * 4, torch.int32, BOX_UNWRITTEN)
    _lib.call("ssv_multicrop_params", bc["B"], bc["hs"], bc["ws"], bc["ncrop"], bc["view_base"], float(bc["scale"][0]), float(bc["scale"][1]), bc["seed"], bc["step"],
              _lib.ptr(d_ids), bc["sample0"] if ids is None else -12345, _lib.ptr(out), _lib.stream())
    buf.verify(what)
    got = out.cpu().numpy().reshape(bc["B"], bc["ncrop"], 4)
    assert not (got == BOX_UNWRITTEN).any(), f"{what}: a box was not written"
    return got


@pytest.mark.parametrize("bc", ao.BOX_CASES, ids=lambda c: c["id"])
def test_boxes_equal_the_restated_draw(lib, bc):
    want, _, margin = ao.box_records(bc)
    assert margin > ao.MARGIN
    t0 = time.perf_counter()
    got = _boxes(bc, bc["id"])
    again = _boxes(bc, bc["id"] + " (second call)")
    _note(bc["id"], (bc["B"], bc["ncrop"], bc["view_base"], bc["hs"], bc["ws"]), got, want, t0)
    np.testing.assert_array_equal(got, again)
    if bc["ids"] is None:
        np.testing.assert_array_equal(got, _boxes(bc, bc["id"] + " (explicit ids)", ids=[bc["sample0"] + k for k in range(bc["B"])]))


# ---- pixels -------------------------------------------------------------------------------------------------------------------------------------------------------------
ENTRY = {"views": "ssv_augment_views", "blur": "ssv_augment_views_blur", "center": "ssv_center_view"}


def _pixels(c, what, entry=None):
    """one guarded call of the case's entry point -> float32 [V, B, Ho, Wo, 3] ([B, Ho, Wo, 3] for the centre view) on the CPU"""
    from ssv_amd import _lib
    ao.check_case(c)
    entry = entry or c.entry
    b, v, hs, ws_, ho, wo = ao.case_shape(c)
    P, lib = _lib.ptr, _lib.load()
    buf = fr.Buffers()
    src = buf.up("src", c.imgs)
    ids = None if c.ids is None else buf.up("ids", c.ids)
    out = buf.out("out", v * b * ho * wo * 3, torch.float32, float("nan"))
    mean, std = _f3(ao.MEAN), _f3(ao.STD)
    if entry == "center":
        _lib.call("ssv_center_view", b, hs, ws_, ho, wo, P(src), P(ids), mean, std, P(out), _lib.stream())
    else:
        params = buf.up("params", c.params)
        sizer, restated = {"views": (lib.ssv_augment_workspace_bytes, ao.workspace_bytes), "blur": (lib.ssv_augment_blur_workspace_bytes, ao.blur_workspace_bytes)}[entry]
        need = sizer(b, v, ho, wo)
        assert need == restated(b, v, ho, wo) > 0
        ws = _workspace(need)
        assert all(t.data_ptr() % 16 == 0 for t in (src, params, out, ws))
        _lib.call(ENTRY[entry], b, v, hs, ws_, ho, wo, P(src), P(ids), P(params), mean, std, P(out), P(ws), need, _lib.stream())
        torch.cuda.synchronize()
        assert bool((ws[need:] == PATTERN).all()), f"{what}: wrote behind its workspace"
    buf.verify(what)
    got = out.cpu().numpy()
    assert not np.isnan(got).any(), f"{what}: an output element was not written"
    return got.reshape(((b,) if entry == "center" else (v, b)) + (ho, wo, 3))


@pytest.mark.parametrize("case", ao.PIXEL_CASES, ids=lambda c: c.id)
def test_pixels_bit_for_bit(lib, case):
    want = ao.reference(case)
    t0 = time.perf_counter()
    got = _pixels(case, case.id)
    again = _pixels(case, case.id + " (second call)")
    _note(case.id, ao.case_shape(case), got, want, t0)
    np.testing.assert_array_equal(got.view(np.int32), again.view(np.int32), err_msg="two calls differ")
    if case.id == "blur.mixed-none":                                      # no record blurred: the bits of the entry point without blur
        np.testing.assert_array_equal(got.view(np.int32), _pixels(case, case.id + " (plain)", entry="views").view(np.int32))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _alloc(entry, base, changed):
    """device buffers that hold the accepted call (and the changed call's source where it is larger); in-bounds records for the smallest source of the two"""
    dim = lambda k: max(base[k], changed[k]) if 0 < changed[k] <= 8192 else base[k]
    r = ao.rng("refuse." + entry)
    bufs, fills = {}, {}
    mean, std = _f3(ao.MEAN), _f3(ao.STD)
    bufs["mean"], bufs["std"] = C.addressof(mean), C.addressof(std)
    keep = [mean, std]
    if entry in ("ssv_augment_params", "ssv_augment_params_blur"):
        fills["params"] = torch.full((dim("nviews") * dim("B") * ao.NPARAM + fr.GUARD,), float("nan"), device="cuda")
    elif entry == "ssv_multicrop_params":
        fills["boxes"] = torch.full((dim("B") * dim("ncrop") * 4 + fr.GUARD,), BOX_UNWRITTEN, dtype=torch.int32, device="cuda")
    else:
        src = torch.from_numpy(r.integers(0, 256, (dim("B"), dim("Hs"), dim("Ws"), 3), dtype=np.uint8)).cuda()
        keep.append(src)
        bufs["src"] = src.data_ptr()
        v = dim("nviews") if "nviews" in base else 1
        fills["out"] = torch.full((v * dim("B") * dim("Ho") * dim("Wo") * 3 + fr.GUARD,), float("nan"), device="cuda")
        if entry != "ssv_center_view":
            hs, ws_ = (min(x for x in (base[k], changed[k]) if x > 0) for k in ("Hs", "Ws"))
            sig = (lambda: float(r.choice([0.0, 1.0]))) if entry.endswith("blur") else (lambda: 0.0)
            recs = np.stack([ao.rand_rec(r, hs, ws_, sigma=sig()) for _ in range(v * dim("B"))])
            params = torch.from_numpy(recs).cuda()
            keep.append(params)
            bufs["params"] = params.data_ptr()
            sizer = ao.workspace_bytes if entry == "ssv_augment_views" else ao.blur_workspace_bytes
            bufs["ws_bytes"] = sizer(base["B"], base["nviews"], base["Ho"], base["Wo"])
            assert bufs["ws_bytes"] == getattr(_lib_(), entry.replace("_views", "") + "_workspace_bytes")(base["B"], base["nviews"], base["Ho"], base["Wo"]) > 0
            fills["ws"] = _workspace(bufs["ws_bytes"])
    for k, t in fills.items():
        bufs[k] = t.data_ptr()
    return bufs, fills, keep


def _lib_():
    from ssv_amd import _lib
    return _lib.load()


def _untouched(fills):
    torch.cuda.synchronize()
    for k, t in fills.items():
        ok = (t == PATTERN).all() if t.dtype == torch.uint8 else (torch.isnan(t).all() if t.is_floating_point() else (t == BOX_UNWRITTEN).all())
        assert bool(ok), f"a refused call wrote to {k}"


@pytest.mark.parametrize("r", ao.REFUSALS, ids=lambda r: r["id"])
def test_refusals_touch_nothing(lib, r):
    from ssv_amd import _lib
    entry = r["entry"]
    base, changed = ao.call_of(r)
    assert ao.verdict(entry, base) == ao.OK and ao.verdict(entry, changed) == r["rc"] != ao.OK
    bufs, fills, keep = _alloc(entry, base, changed)
    fn = getattr(lib, entry)
    t0 = time.perf_counter()
    rc = fn(*ao.marshal(entry, changed, bufs.__getitem__, _lib.stream()))
    msg = lib.ssv_last_error().decode()
    assert rc == r["rc"], (rc, msg)
    inner = "ssv_augment_params" if entry == "ssv_augment_params_blur" and isinstance(r["change"].get("cfg"), dict) else entry      # refused by the entry point the blur one calls
    assert msg.startswith(inner + ":"), msg
    _untouched(fills)
    rc = fn(*ao.marshal(entry, base, bufs.__getitem__, _lib.stream()))     # the unchanged call is accepted afterwards, and writes every output element
    assert rc == ao.OK, (rc, lib.ssv_last_error().decode())
    torch.cuda.synchronize()
    name = "params" if "params" in fills else ("boxes" if "boxes" in fills else "out")
    n = {"params": lambda: base["nviews"] * base["B"] * ao.NPARAM, "boxes": lambda: base["B"] * base["ncrop"] * 4,
         "out": lambda: base.get("nviews", 1) * base["B"] * base["Ho"] * base["Wo"] * 3}[name]()
    head, tail = fills[name][:n], fills[name][n:]
    assert bool((~torch.isnan(head)).all() if head.is_floating_point() else (head != BOX_UNWRITTEN).all()), "the accepted call left an output element unwritten"
    assert bool(torch.isnan(tail).all() if tail.is_floating_point() else (tail == BOX_UNWRITTEN).all()), "the accepted call wrote behind its output"
    assert "ws" not in fills or bool((fills["ws"][bufs["ws_bytes"]:] == PATTERN).all())
    REPORT[r["id"]] = {"label": r["label"], "shape": [str(r["change"])], "elements": 1, "mismatches": 0, "seconds": round(time.perf_counter() - t0, 4)}


def test_size_functions_answer_refused_shapes_with_zero(lib):
    for shape in ao.WORKSPACE_REFUSALS:
        assert lib.ssv_augment_workspace_bytes(*shape) == 0 == lib.ssv_augment_blur_workspace_bytes(*shape)
    for shape in ao.BLUR_WORKSPACE_REFUSALS:
        assert lib.ssv_augment_blur_workspace_bytes(*shape) == 0 < lib.ssv_augment_workspace_bytes(*shape)


# ---- the front end ------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_front_end_pass(lib):
    """GpuTransform.draw / apply / one_view and MultiCrop.__call__ once each on the views.crop inputs; without color_jitter, random_gray or random_flip the chain
    equals the restatement with that probability at 0"""
    from ssv_amd import ops
    from ssv_amd.utils import augmentations
    case = ao.PIXEL_BY_ID["views.crop-8x10"]
    ao.check_case(case)
    b, v, hs, ws_, ho, wo = ao.case_shape(case)
    dev = torch.device("cuda:0")
    imgs, idx = torch.from_numpy(case.imgs).to(dev), torch.from_numpy(case.ids).to(dev)
    t0 = time.perf_counter()
    compared = 0
    for drop in ao.FRONT_DROPS:
        tf = augmentations.get_transform(ao.front_chain(case.out_hw, drop))
        want, margin = ao.front_records(case.ids, hs, ws_, drop)
        assert margin > ao.MARGIN
        params = tf.draw(imgs, idx, ao.STEP)
        np.testing.assert_array_equal(params.cpu().numpy().view(np.int32), want.view(np.int32), err_msg=f"draw without {drop}")
        assert drop is None or (want[..., {"color_jitter": 0, "random_gray": 9, "random_flip": 14}[drop]] == 0).all()
        views = tf.apply(imgs, idx, params)
        assert views.shape == (2, b, 3, ho, wo)
        ref = np.stack([np.stack([ao.view(case.imgs[int(i)], want[vi, k], case.out_hw) for k, i in enumerate(case.ids)]) for vi in range(2)])
        np.testing.assert_array_equal(views.permute(0, 1, 3, 4, 2).contiguous().cpu().numpy().view(np.int32), ref.view(np.int32), err_msg=f"apply without {drop}")
        compared += want.size + ref.size
    tf = augmentations.get_transform(ao.front_chain(case.out_hw))
    own = tf.apply(imgs, idx, torch.from_numpy(case.params).to(dev))          # the case's own records through the front end
    np.testing.assert_array_equal(own.permute(0, 1, 3, 4, 2).contiguous().cpu().numpy().view(np.int32), ao.reference(case).view(np.int32))
    te = augmentations.get_transform({"center_crop": {"size": list(case.out_hw)}, "to_tensor": None, "normalize": {"mean": ao.MEAN, "std": ao.STD}})
    one = te.one_view(imgs, idx).permute(0, 2, 3, 1).contiguous().cpu().numpy()
    np.testing.assert_array_equal(one.view(np.int32), np.stack([ao.center_view(case.imgs[int(i)], case.out_hw) for i in case.ids]).view(np.int32))
    # MultiCrop: its boxes are the restated draws, so its crops are ssv_multicrop of its own views at those boxes, bit for bit
    mc = augmentations.MultiCrop(dict(ao.MULTICROP, train_transforms=ao.front_chain(case.out_hw)))
    crops = mc(imgs, idx, ao.STEP)
    views = tf.apply(imgs, idx, tf.draw(imgs, idx, ao.STEP))
    for copy in range(2):
        for kind, size in (("global", ao.MULTICROP["global_size"]), ("local", ao.MULTICROP["local_size"])):
            boxes, margin = ao.front_boxes(case.ids, ho, wo, copy, kind)
            assert margin > ao.MARGIN and (boxes[..., 0] + boxes[..., 2] <= ho).all() and (boxes[..., 1] + boxes[..., 3] <= wo).all() and (boxes >= 0).all()
            ncrop, scale, base = boxes.shape[1], ((0.3, 1.0) if kind == "global" else (0.08, 0.3)), (16 if kind == "global" else 144) + 256 * copy
            drawn = ops.multicrop_params(b, ho, wo, ncrop, base, scale, ao.SEED, ao.STEP, sample_ids=idx)
            np.testing.assert_array_equal(drawn.cpu().numpy(), boxes)
            want = ops.multicrop(views[copy].permute(0, 2, 3, 1), torch.from_numpy(boxes).to(dev), tuple(size)).permute(0, 1, 4, 2, 3)
            got = crops[f"{kind}_{copy + 1}"]
            assert got.shape == (b, ncrop, 3) + tuple(size) and torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32)), (kind, copy)
            compared += boxes.size + got.numel()
    REPORT["front.end"] = {"label": "front.end", "shape": list(ao.case_shape(case)), "elements": int(compared), "mismatches": 0, "seconds": round(time.perf_counter() - t0, 4)}
