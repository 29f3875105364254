"""TEST INFRASTRUCTURE shared by tests/test_augment_forms_cpu.py (no GPU) and tests/test_gpu_augment_forms.py: the case tables, the seeded generators and the
numpy restatements behind the launch-form tests of csrc/augment.hip.  Both files import this module, so they see the same bytes.

  * the plan          KMAX, the 256-thread grid-stride launches capped at 8192 blocks, the 64-thread parameter blocks, the four LDS classes of the blur kernel
                      and the acceptance rule of the resampler, restated; tests/test_augment_forms_cpu.py holds them against the source text;
  * the draws         `sample_rrc` on oracle.augment._Stream, with the branch taken (accept / wide / tall / whole) and the smallest distance of any drawn
                      quantity from a decision boundary; `draw_record` (the 16-float record of ssv_augment_params[_blur]) and `draw_boxes` (ssv_multicrop_params);
  * the pixels        `view`: the chain of oracle.augment.view_numpy / blur_oracle.view_numpy_blur written the way the kernels walk it (both resampling passes
                      always, at most KMAX taps, NHWC out), with keyword switches for deliberately WRONG variants (MUTANTS) that only the sensitivity test of the
                      GPU-free file uses; unmutated it is held bit for bit against both older restatements and against Pillow there; `center_view`;
  * the cases         PIXEL_CASES, PARAM_CASES, BOX_CASES, REFUSALS: every input the GPU file passes to the library.  `check_case` proves a pixel case safe
                      to launch (crop boxes inside the source, order slots a permutation of 0..3, ids inside the image stack): the library cannot validate
                      device-resident records.
"""
import itertools
import math
import zlib
from collections import namedtuple

import numpy as np

import blur_oracle as bo
from oracle import augment as A

# ------------------------------------------------------------------------------------------- the plan, restated
ENTRY_POINTS = ("ssv_augment_params", "ssv_augment_params_blur", "ssv_augment_views", "ssv_augment_views_blur", "ssv_augment_blur_workspace_bytes",
                "ssv_augment_workspace_bytes", "ssv_center_view", "ssv_multicrop_params")
NPARAM, KMAX, THREADS, GRID_CAP, PARAM_THREADS = 16, 8, 256, 8192, 64
MAX_TAPS = 6                                                                       # what the acceptance rule lets through: src <= 3 out, six pixel centres under the triangle
BLUR_CLASSES = ((8192, 256), (32768, 512), (65536, 1024), (163840, 1024))        # (LDS bytes, threads); chosen by plane2 <= bytes, the last takes the rest
BLUR_MAX_PIXELS, BLUR_MAX_SIGMA, BLUR_STAGE_ALIGN = 81920, 1000.0, 256
MAX_SOURCE_PIXELS = 1 << 24                                                        # Hs * Ws must stay below it
OK, ERR_INVALID, ERR_WORKSPACE = 0, -1, -2
MEAN, STD = [0.4914, 0.4822, 0.4465], [0.2470, 0.2435, 0.2616]
SEED, STEP = 420, 7
MARGIN = 1e-9                                                                      # no drawn quantity of any case may lie this close to a decision boundary
DEFAULT_CFG = dict(brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1, p_jitter=0.8, p_gray=0.2, p_flip=0.5, scale_min=0.2, scale_max=1.0,
                   ratio_min=3.0 / 4.0, ratio_max=4.0 / 3.0)
CFG_FIELDS = tuple(DEFAULT_CFG)


def trips(pixels):
    """trips of the grid-stride loop of aug_views_k / center_view_k for `pixels` output pixels"""
    blocks = min(max(-(-pixels // THREADS), 1), GRID_CAP)
    return -(-pixels // (blocks * THREADS))


def accepted(src, out):
    """the resampler's acceptance rule along one axis, in the integer arithmetic of the source"""
    return 2 * (src + out - 1) // out + 1 <= KMAX


def blur_class(ho, wo):
    """(class 1..4, LDS bytes, threads, whether the 16-byte vector fill runs)"""
    n = ho * wo
    plane2 = 2 * ((n + 15) // 16 * 16)
    k = next((i for i, (lds, _) in enumerate(BLUR_CLASSES[:3]) if plane2 <= lds), 3)
    return k + 1, BLUR_CLASSES[k][0], BLUR_CLASSES[k][1], n % 16 == 0


def workspace_bytes(b, v, ho, wo):
    return 0 if min(b, v, ho, wo) <= 0 else v * b * (1 + (ho + wo) * (2 + KMAX)) * 4


def blur_workspace_bytes(b, v, ho, wo):
    if min(b, v, ho, wo) <= 0 or ho * wo > BLUR_MAX_PIXELS:
        return 0
    base = -(-workspace_bytes(b, v, ho, wo) // BLUR_STAGE_ALIGN) * BLUR_STAGE_ALIGN
    return base + v * b * 3 * ho * wo


def center_offset(d, half_up=False):
    """torchvision center_crop: int(round(d / 2.0)), Python's round-half-to-even"""
    return (d + 1) // 2 if half_up else int(round(d / 2.0))


# ------------------------------------------------------------------------------------------- the draws
def _near(x):
    """distance of x from the nearest integer"""
    return abs(x - round(x))


def sample_rrc(st, hs, ws, smin, smax, rmin, rmax):
    """RandomResizedCrop.get_params as csrc/augment.hip sample_rrc draws it -> ((top, left, h, w), branch, margin)"""
    area, margin = float(hs * ws), math.inf
    lr0, lr1 = math.log(rmin), math.log(rmax)
    for _ in range(10):
        target = area * (smin + st.uniform() * (smax - smin))
        ratio = math.exp(lr0 + st.uniform() * (lr1 - lr0))
        xw, xh = math.sqrt(target * ratio) + 0.5, math.sqrt(target / ratio) + 0.5
        margin = min(margin, _near(xw), _near(xh))
        w, h = int(math.floor(xw)), int(math.floor(xh))
        ui, uj = st.uniform(), st.uniform()
        if 0 < w <= ws and 0 < h <= hs:
            yi, yj = ui * (hs - h + 1), uj * (ws - w + 1)
            margin = min(margin, yi - math.floor(yi), math.floor(yi) + 1 - yi, yj - math.floor(yj), math.floor(yj) + 1 - yj)
            return (int(yi), int(yj), h, w), "accept", margin
    in_ratio = ws / hs
    if in_ratio < rmin:
        x = ws / rmin + 0.5
        w, h, branch, margin = ws, int(math.floor(x)), "tall", min(margin, _near(x))
    elif in_ratio > rmax:
        x = hs * rmax + 0.5
        h, w, branch, margin = hs, int(math.floor(x)), "wide", min(margin, _near(x))
    else:
        w, h, branch = ws, hs, "whole"
    return ((hs - h) // 2, (ws - w) // 2, h, w), branch, margin


def draw_record(seed, step, sample, view, hs, ws, cfg=None, blur=None):
    """One record of ssv_augment_params (blur = None: slot [15] is 0) or ssv_augment_params_blur (blur = (p, lo, hi)) -> (float32 [16], branch, margin)"""
    c = dict(DEFAULT_CFG, **(cfg or {}))
    st = A._Stream(seed, step, sample, view)
    p = np.zeros(NPARAM, np.float32)
    u = st.uniform()
    p[0], margin = (1.0 if u < c["p_jitter"] else 0.0), abs(u - c["p_jitter"])
    order = [0, 1, 2, 3]
    for i in range(3, 0, -1):
        y = st.uniform() * (i + 1)
        margin = min(margin, y - math.floor(y), math.floor(y) + 1 - y)
        order[i], order[int(y)] = order[int(y)], order[i]
    p[1:5] = order
    for slot, key in ((5, "brightness"), (6, "contrast"), (7, "saturation")):
        lo = max(0.0, 1.0 - c[key])
        p[slot] = np.float32(lo + st.uniform() * (1.0 + c[key] - lo))
    p[8] = np.float32(-c["hue"] + st.uniform() * 2.0 * c["hue"])
    u = st.uniform()
    p[9], margin = (1.0 if u < c["p_gray"] else 0.0), min(margin, abs(u - c["p_gray"]))
    box, branch, m = sample_rrc(st, hs, ws, c["scale_min"], c["scale_max"], c["ratio_min"], c["ratio_max"])
    p[10:14] = box
    u = st.uniform()
    p[14], margin = (1.0 if u < c["p_flip"] else 0.0), min(margin, m, abs(u - c["p_flip"]))
    if blur is not None:
        sb = A._Stream(seed, step, sample, bo.BLUR_VIEW_BASE + view)
        u0, u1 = sb.uniform(), sb.uniform()
        p[15], margin = (np.float32(blur[1] + u1 * (blur[2] - blur[1])) if u0 < blur[0] else 0.0), min(margin, abs(u0 - blur[0]))
    return p, branch, margin


def draw_boxes(seed, step, sample, view_base, crop, hs, ws, scale):
    """One box of ssv_multicrop_params: the crop draw alone on the stream keyed (seed, step, sample, view_base + crop), ratio 3/4 .. 4/3"""
    return sample_rrc(A._Stream(seed, step, sample, view_base + crop), hs, ws, scale[0], scale[1], 3.0 / 4.0, 4.0 / 3.0)


# ------------------------------------------------------------------------------------------- the pixels
MUTANTS = {"center_half_up": "center.round", "mean_trunc": "views.mean", "blend_noclip": "views.order", "flip_off_by_one": "views.out", "taps6": "views.crop", "taps5": "views.crop",
           "mean_after_chain": "views.order", "hue_nowrap": "views.colours", "blur_no_edge_repeat": "blur.class"}
UNOBSERVABLE = {"taps6"}                                                            # equal bits at every accepted shape (tests/test_augment_forms_cpu.py proves it): no case can notice it


def _blend(deg, img, factor, noclip=False, stats=None):
    a = np.float32(factor)
    d, i = deg.astype(np.int32), img.astype(np.int32)
    t = (d.astype(np.float32) + a * (i - d).astype(np.float32)).astype(np.float32)
    if 0.0 <= float(a) <= 1.0 or noclip:
        return t.astype(np.int32).astype(np.uint8)
    if stats is not None:
        stats["low"] = stats.get("low", 0) + int((t <= 0).sum())
        stats["high"] = stats.get("high", 0) + int((t >= 255).sum())
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32))).astype(np.uint8)


def hue_shift_of(p, wrap=True):
    s = int(float(np.float32(p[8])) * 255)
    return s % 256 if wrap else s


def _one_op(op, img, p, mutant, stats):
    """an op of the jitter chain other than contrast"""
    noclip = mutant == "blend_noclip"
    if op == 0:
        return _blend(np.zeros_like(img), img, p[5], noclip, stats)
    if op == 2:
        return _blend(np.repeat(A._gray_l(img)[..., None], 3, -1).astype(np.uint8), img, p[7], noclip, stats)
    hsv = A._rgb2hsv(img)
    h = hsv[..., 0].astype(np.int32) + hue_shift_of(p, mutant != "hue_nowrap")
    hsv[..., 0] = (np.clip(h, 0, 255) if mutant == "hue_nowrap" else h % 256).astype(np.uint8)
    if stats is not None:
        stats.setdefault("sectors", set()).update(np.unique(np.floor(hsv[..., 0].astype(np.float64) * 6.0 / 255.0).astype(np.int64)[hsv[..., 1] > 0] % 6).tolist())
    return A._hsv2rgb(hsv)


def prefix_luma(img, p):
    """the luma image in front of the contrast op of record p: what aug_prep_k averages"""
    for op in (int(p[k]) for k in range(1, 5)):
        if op == 1:
            break
        img = _one_op(op, img, p, None, None)
    return A._gray_l(img)


def color_ops(img, p, mutant=None, stats=None):
    first = img
    if p[0] >= 0.5:
        ops = [int(p[k]) for k in range(1, 5)]
        for op in ops:
            if op != 1:
                img = _one_op(op, img, p, mutant, stats)
                continue
            base = img
            if mutant == "mean_after_chain":
                base = first
                for other in ops:
                    if other != 1:
                        base = _one_op(other, base, p, None, None)
            l = A._gray_l(base)
            mean = int(l.sum() / l.size) if mutant == "mean_trunc" else int(l.sum() / l.size + 0.5)
            img = _blend(np.full_like(img, mean), img, p[6], mutant == "blend_noclip", stats)
    if p[9] >= 0.5:
        img = np.repeat(A._gray_l(img)[..., None], 3, -1).astype(np.uint8)
    return img


def coeffs(in_size, out_size, kmax=KMAX):
    """coeffs_for of csrc/augment.hip for every output index: the tap count is capped at kmax BEFORE the weights are summed -> (xmin, count, kk [out, kmax])"""
    scale = in_size / out_size
    support = max(scale, 1.0)
    ss = 1.0 / support
    xmins, counts, kk = np.zeros(out_size, np.int64), np.zeros(out_size, np.int64), np.zeros((out_size, kmax), np.int64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(min(int(center + support + 0.5), in_size) - xmin, kmax)
        w = [max(1.0 - abs((x + xmin - center + 0.5) * ss), 0.0) for x in range(n)]
        ww = sum(w)
        xmins[xx], counts[xx] = xmin, n
        for x in range(n):
            kk[xx, x] = int((w[x] / ww if ww != 0.0 else w[x]) * (1 << A._PRECISION_BITS) + 0.5)
    return xmins, counts, kk


def _pass(x, in_size, out_size, kmax):
    """one resampling pass along axis 0 of an int64 [in, n, 3] image -> uint8 range [out, n, 3]"""
    xmins, counts, kk = coeffs(in_size, out_size, kmax)
    t = max(int(counts.max()), 1)
    idx = np.minimum(xmins[:, None] + np.arange(t)[None, :], in_size - 1)              # taps past the count carry a zero coefficient
    acc = (x[idx] * kk[:, :t, None, None]).sum(1) + (1 << (A._PRECISION_BITS - 1))
    return np.clip(acc >> A._PRECISION_BITS, 0, 255)


def resize(img, out_hw, kmax=KMAX):
    """both passes, always (the kernel has no identity shortcut): horizontal, uint8, vertical"""
    h, w = img.shape[:2]
    x = _pass(img.astype(np.int64).transpose(1, 0, 2), w, out_hw[1], kmax).transpose(1, 0, 2)
    return _pass(x, h, out_hw[0], kmax).astype(np.uint8)


def line_pass(img, radius, ww, fw, repeat=True):
    """blur_oracle.line_pass with a switch: repeat = False reads 0 outside the line instead of the edge pixel"""
    n = img.shape[-1]
    x = np.concatenate([img.astype(np.int64), np.zeros(img.shape[:-1] + (1,), np.int64)], -1)       # index n: the 0 of the mutant
    pos = np.arange(n)
    at = (lambda i: x[..., np.clip(i, 0, n - 1)]) if repeat else (lambda i: x[..., np.where((i < 0) | (i >= n), n, i)])
    acc = sum(at(pos + d) for d in range(-radius, radius + 1))
    edge = at(pos - radius - 1) + at(pos + radius + 1)
    return (((ww * acc + fw * edge + (1 << 23)) & 0xFFFFFFFF) >> 24).astype(np.uint8)


def gaussian_blur(img, sigma, repeat=True):
    sc = bo.scalars(sigma) if sigma > 0 else None
    if sc is None:
        return img.copy()
    x = np.moveaxis(img, 1, -1)
    for _ in range(3):
        x = line_pass(x, *sc, repeat=repeat)
    x = np.moveaxis(np.moveaxis(x, -1, 1), 0, -1)
    for _ in range(3):
        x = line_pass(x, *sc, repeat=repeat)
    return np.ascontiguousarray(np.moveaxis(x, -1, 0))


def normalise(u8):
    t = u8.astype(np.float32) / np.float32(255)
    return np.ascontiguousarray((t - np.asarray(MEAN, np.float32)) / np.asarray(STD, np.float32))


def view(img, p, out_hw, blur=False, mutant=None, stats=None):
    """one view, float32 [Ho, Wo, 3] (NHWC, as the kernels write it); blur: whether slot [15] is read (the *_blur entry points)"""
    assert mutant is None or mutant in MUTANTS
    x = color_ops(np.ascontiguousarray(img), p, mutant, stats)
    top, left, ch, cw = (int(v) for v in p[10:14])
    x = resize(x[top:top + ch, left:left + cw], out_hw, {"taps6": 6, "taps5": 5}.get(mutant, KMAX))
    if p[14] >= 0.5:
        x = np.roll(x[:, ::-1], 1, axis=1) if mutant == "flip_off_by_one" else x[:, ::-1]
    if blur and p[15] > 0:
        x = gaussian_blur(np.ascontiguousarray(x), np.float32(p[15]), mutant != "blur_no_edge_repeat")
    return normalise(x)


def center_view(img, out_hw, mutant=None):
    h, w = img.shape[:2]
    top, left = center_offset(h - out_hw[0], mutant == "center_half_up"), center_offset(w - out_hw[1], mutant == "center_half_up")
    return normalise(img[top:top + out_hw[0], left:left + out_hw[1]])


# ------------------------------------------------------------------------------------------- seeded generators
def rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def images(name, n, hs, ws):
    """n uint8 images: random, then (cyclically) a grey one, one of four levels per channel, a smooth ramp, and a random one again"""
    r = rng("img." + name)
    out = r.integers(0, 256, (n, hs, ws, 3), dtype=np.uint8)
    for k in range(n):
        if k % 5 == 1:
            out[k] = out[k][:, :, :1]
        elif k % 5 == 2:
            out[k] = (out[k] // 85) * 85
        elif k % 5 == 3:
            out[k] = ((np.arange(hs)[:, None, None] * 7 + np.arange(ws)[None, :, None] * 5 + np.arange(3)[None, None, :] * 60) % 256).astype(np.uint8)
    return out


def lattice():
    """512 x 512: every colour of a 64-level lattice per channel, the levels holding both ends of the range"""
    lv = np.array(sorted([0, 1, 2, 253, 254, 255] + np.linspace(6, 249, 58).round().astype(int).tolist()), np.int64)
    assert len(set(lv.tolist())) == 64
    i = np.arange(64 ** 3)
    return np.stack([lv[i >> 12], lv[(i >> 6) & 63], lv[i & 63]], -1).astype(np.uint8).reshape(512, 512, 3)


def rec(box, jitter=0, order=(0, 1, 2, 3), f=(1.0, 1.0, 1.0, 0.0), gray=0, flip=0, sigma=0.0):
    p = np.zeros(NPARAM, np.float32)
    p[0], p[1:5], p[5:9], p[9], p[10:14], p[14], p[15] = jitter, order, f, gray, box, flip, sigma
    return p


def rand_box(r, hs, ws):
    h, w = int(r.integers(1, hs + 1)), int(r.integers(1, ws + 1))
    return int(r.integers(0, hs - h + 1)), int(r.integers(0, ws - w + 1)), h, w


def rand_rec(r, hs, ws, box=None, jitter=None, flip=None, sigma=0.0):
    return rec(box or rand_box(r, hs, ws), int(r.random() < 0.8) if jitter is None else jitter, r.permutation(4),
               tuple(r.uniform(0.6, 1.4, 3)) + (r.uniform(-0.1, 0.1),), int(r.random() < 0.2), int(r.random() < 0.5) if flip is None else flip, sigma)


# ------------------------------------------------------------------------------------------- the pixel cases
Case = namedtuple("Case", "id label entry imgs ids params out_hw")        # entry: views | blur | center; params [V, B, 16] (center: None); ids int64 [B] or None


def case_shape(c):
    """(B, V, Hs, Ws, Ho, Wo)"""
    b = len(c.ids) if c.ids is not None else len(c.imgs)
    return (b, 1 if c.params is None else c.params.shape[0]) + tuple(c.imgs.shape[1:3]) + tuple(c.out_hw)


def _random_case(cid, label, n, src, out, b=None, v=2, ids=None, entry="views", sigmas=None, **kw):
    r = rng(cid)
    b = b or (len(ids) if ids is not None else n)
    p = np.stack([[rand_rec(r, src[0], src[1], **kw) for _ in range(b)] for _ in range(v)])
    if sigmas is not None:
        p[..., 15] = np.asarray(sigmas, np.float32)
    return Case(cid, label, entry, images(cid, n, *src), None if ids is None else np.asarray(ids, np.int64), p, out)


ORDERS = list(itertools.permutations(range(4)))
FACTOR_SETS = ((1.8, 1.8, 1.8, 0.5), (0.0, 0.0, 0.0, -0.5), (0.6, 1.3, 0.7, 0.08), (1.0, 0.5, 1.5, -0.03))
HUE_FACTORS = (0.0, 1.5 / 255, -1.5 / 255, 0.5, -0.5)                      # shifts 0, +1, -1 (255), 127, -127 (129)
CROP_BOXES = ((0, 0, 24, 30), (0, 0, 1, 1), (0, 29, 1, 1), (23, 0, 1, 1), (23, 29, 1, 1), (5, 0, 1, 30), (0, 7, 24, 1), (3, 4, 2, 3), (16, 20, 8, 10),
              (0, 0, 24, 10), (0, 0, 8, 30), (1, 1, 23, 29))                               # on a 24 x 30 source; to 8 x 10: x3 on both axes (6 taps, the last of weight 0), identity, x3 on one axis,
                                                                           # x2.9: six taps that all count
ROUND_DIFFS = (0, 1, 2, 3, 6, 7)
BLUR_CLASS_OUTS = ((64, 64), (65, 63), (64, 65), (128, 128), (128, 129), (181, 181), (182, 181), (320, 256))


def _build():
    cases = []
    # views.order: 24 orders (samples) x 4 factor sets x grey off / on (views), jitter on
    r = rng("views.order")
    p = np.stack([[rec(rand_box(r, 21, 18), 1, o, f, g, int(r.random() < 0.5)) for o in ORDERS] for f in FACTOR_SETS for g in (0, 1)])
    cases.append(Case("views.order", "views.order", "views", images("views.order", 24, 21, 18), None, p, (8, 7)))
    # views.colours: the lattice, all-0, all-255 and a grey ramp; five hue shifts as views; identity crop; factors 1 leave the other ops exact
    imgs = np.stack([lattice(), np.zeros((512, 512, 3), np.uint8), np.full((512, 512, 3), 255, np.uint8),
                     np.repeat(((np.arange(512)[:, None] + np.arange(512)[None, :]) // 4).astype(np.uint8)[..., None], 3, -1)])
    p = np.stack([[rec((0, 0, 512, 512), 1, ORDERS[(5 * v + 1) % 24], (1.0, 1.0, 1.0, h), 0, int(v == 3)) for _ in range(4)] for v, h in enumerate(HUE_FACTORS)])
    cases.append(Case("views.colours", "views.colours", "views", imgs, None, p, (512, 512)))
    # views.crop: the edge boxes to 8 x 10 (down) and to 32 x 32 (up)
    for out in ((8, 10), (32, 32)):
        cid = f"views.crop-{out[0]}x{out[1]}"
        r = rng(cid)
        p = np.stack([[rand_rec(r, 24, 30, box=b) for b in CROP_BOXES] for _ in range(2)])
        cases.append(Case(cid, "views.crop", "views", images(cid, 4, 24, 30), np.arange(len(CROP_BOXES), dtype=np.int64) % 4, p, out))
    # views.out: Ho != Wo with an odd Wo, Wo = 1, 1 x 1; view 0 flipped, view 1 not
    for src, out in (((12, 20), (5, 9)), ((14, 3), (7, 1)), ((3, 3), (1, 1))):
        cid = f"views.out-{out[0]}x{out[1]}"
        c = _random_case(cid, "views.out", 3, src, out)
        c.params[0, :, 14], c.params[1, :, 14] = 1, 0
        cases.append(c)
    cases.append(_random_case("views.tabs-3x260", "views.tabs", 2, (9, 300), (3, 260), v=1))
    # views.mean: 1 x 2 grey pairs (g, g + 1): luma mean g + 0.5 in front of the contrast op (first, or behind a brightness of exactly 1)
    imgs = np.stack([np.repeat(np.array([[g, g + 1]], np.uint8)[..., None], 3, -1) for g in (10, 127, 254)])
    p = np.stack([[rec((0, 0, 1, 2), 1, (1, 0, 2, 3), (0.7, 0.5, 1.2, 0.05)) for _ in range(3)], [rec((0, 0, 1, 2), 1, (0, 1, 2, 3), (1.0, 1.7, 0.8, 0.0)) for _ in range(3)]])
    cases.append(Case("views.mean-1x2", "views.mean", "views", imgs, None, p, (2, 3)))
    cases.append(_random_case("views.mean-5x7", "views.mean", 2, (5, 7), (4, 4), jitter=1))
    cases.append(_random_case("views.mean-17x19", "views.mean", 2, (17, 19), (8, 8), jitter=1))
    # views.stride: 2 * 41 * 160 * 160 = 2 099 200 pixels; ids and records cycle over 4, so 8 distinct views
    c = _random_case("views.stride", "views.stride", 4, (48, 40), (160, 160), ids=np.arange(41) % 4)
    cases.append(c._replace(params=np.ascontiguousarray(c.params[:, np.arange(41) % 4])))
    cases.append(_random_case("views.ids-null", "views.ids", 6, (10, 12), (6, 6), v=1))
    cases.append(_random_case("views.ids-perm", "views.ids", 6, (10, 12), (6, 6), ids=[5, 3, 3, 0, 1, 5, 2, 4, 0]))
    cases.append(_random_case("views.ids-v5", "views.ids", 6, (10, 12), (6, 6), v=5, ids=[2, 2, 0, 5]))
    # blur
    for out in BLUR_CLASS_OUTS:
        cases.append(_random_case(f"blur.class-{out[0]}x{out[1]}", "blur.class", 2, (40, 36), out, entry="blur", sigmas=[[0.3, 2.0], [8.0, 0.0]]))
    cases.append(_random_case("blur.thin-1x40", "blur.thin", 2, (3, 36), (1, 40), entry="blur", sigmas=[[2.0, 0.3], [0.0, 8.0]]))
    cases.append(_random_case("blur.thin-40x1", "blur.thin", 2, (36, 3), (40, 1), entry="blur", sigmas=[[2.0, 0.3], [0.0, 8.0]]))
    cases.append(_random_case("blur.mixed-all", "blur.mixed", 3, (20, 24), (16, 12), entry="blur", sigmas=[[0.3, 1.1, 2.0], [3.7, 8.0, 0.5]]))
    cases.append(_random_case("blur.mixed-none", "blur.mixed", 3, (20, 24), (16, 12), entry="blur", sigmas=[[0.0] * 3] * 2))
    # centre view
    for dh in ROUND_DIFFS:
        for dw in ROUND_DIFFS:
            cid = f"center.round-d{dh}x{dw}"
            cases.append(Case(cid, "center.round", "center", images(cid, 2, 4 + dh, 5 + dw), None, None, (4, 5)))
    cases.append(Case("center.stride", "center.stride", "center", images("center.stride", 3, 257, 259), np.arange(33, dtype=np.int64) % 3, None, (256, 256)))
    cases.append(Case("center.ids-null", "center.ids", "center", images("center.ids", 5, 9, 8), None, None, (6, 6)))
    cases.append(Case("center.ids-perm", "center.ids", "center", images("center.ids", 5, 9, 8), np.array([4, 0, 0, 3, 1, 2, 4], np.int64), None, (6, 6)))
    return cases


PIXEL_CASES = _build()
PIXEL_BY_ID = {c.id: c for c in PIXEL_CASES}
assert len(PIXEL_BY_ID) == len(PIXEL_CASES)


def check_case(c):
    """everything the library cannot check of device-resident inputs: never launch a case that fails this"""
    b, v, hs, ws, ho, wo = case_shape(c)
    n = len(c.imgs)
    assert c.imgs.dtype == np.uint8 and c.imgs.shape == (n, hs, ws, 3) and min(b, v, hs, ws, ho, wo) > 0
    assert c.ids is None or (c.ids.dtype == np.int64 and c.ids.shape == (b,) and 0 <= c.ids.min() and c.ids.max() < n)
    assert c.ids is not None or b <= n
    if c.entry == "center":
        assert c.params is None and hs >= ho and ws >= wo
        return
    p = c.params
    assert p.dtype == np.float32 and p.shape == (v, b, NPARAM) and np.isfinite(p).all()
    assert (np.sort(p[..., 1:5], -1) == np.arange(4)).all(), "an order slot outside 0..3"
    top, left, h, w = (p[..., k] for k in range(10, 14))
    assert (p[..., 10:14] == np.floor(p[..., 10:14])).all() and (top >= 0).all() and (left >= 0).all() and (h >= 1).all() and (w >= 1).all()
    assert (top + h <= hs).all() and (left + w <= ws).all(), "a crop box leaves the source"
    assert accepted(hs, ho) and accepted(ws, wo) and hs * ws < MAX_SOURCE_PIXELS
    assert (p[..., 15] >= 0).all() and (p[..., 15] <= BLUR_MAX_SIGMA).all() and (c.entry == "blur" or (p[..., 15] == 0).all())
    assert c.entry != "blur" or ho * wo <= BLUR_MAX_PIXELS


def distinct_views(c):
    """{(image number, record bytes): (image, record)}: what a case's reference has to compute"""
    b, v = case_shape(c)[:2]
    out = {}
    for vi in range(v):
        for k in range(b):
            i = int(c.ids[k]) if c.ids is not None else k
            key = (i, b"" if c.params is None else c.params[vi, k].tobytes())
            out.setdefault(key, (c.imgs[i], None if c.params is None else c.params[vi, k]))
    return out


_REFS = {}


def reference(c, mutant=None, stats=None):
    """float32 [V, B, Ho, Wo, 3] ([B, Ho, Wo, 3] for the centre view); computed once per case, shared, read-only"""
    if mutant is None and stats is None and c.id in _REFS:
        return _REFS[c.id]
    done = {key: (center_view(img, c.out_hw, mutant) if c.entry == "center" else view(img, p, c.out_hw, c.entry == "blur", mutant, stats))
            for key, (img, p) in distinct_views(c).items()}
    b, v = case_shape(c)[:2]
    rows = [[done[(int(c.ids[k]) if c.ids is not None else k, b"" if c.params is None else c.params[vi, k].tobytes())] for k in range(b)] for vi in range(v)]
    out = np.stack([np.stack(r) for r in rows])
    out = out[0] if c.entry == "center" else out
    if mutant is None and stats is None:
        out.setflags(write=False)
        _REFS[c.id] = out
    return out


# ------------------------------------------------------------------------------------------- the parameter and box cases
def _cfg(**kw):
    return dict(DEFAULT_CFG, **kw)


TAILS = ((1, 1), (63, 1), (32, 2), (65, 1), (13, 5), (9, 16))            # (B, V): 1, 63, 64, 65 (twice) and 144 records against blocks of 64
RRC_SOURCES = (((8, 64), (0.9, 1.0), "wide"), ((64, 8), (0.9, 1.0), "tall"), ((30, 40), (1.0, 1.0), "whole"))
BIG_IDS = [(1 << 32) + 5, (1 << 48) + 5, 5]                                # the counter holds 48 bits of the id: the last two share a stream


def _pcase(cid, label, b, v, hw=(40, 36), cfg=None, seed=SEED, step=STEP, ids=None, sample0=0, blur=None):
    return dict(id=cid, label=label, B=b, V=v, hs=hw[0], ws=hw[1], cfg=cfg or dict(DEFAULT_CFG), seed=seed, step=step,
                ids=None if ids is None else [int(i) for i in ids], sample0=sample0, blur=blur)


PARAM_CASES = [_pcase(f"params.tail-{b}x{v}", "params.tail", b, v) for b, v in TAILS] + [
    _pcase("params.ids-sample0", "params.ids", 5, 2, sample0=1000),
    _pcase("params.ids-explicit", "params.ids", 5, 2, ids=1000 + np.arange(5)),
    _pcase("params.ids-big", "params.ids", 3, 2, ids=BIG_IDS),
    _pcase("params.ids-step", "params.ids", 5, 2, step=(1 << 32) + 7),
    _pcase("params.ids-seed", "params.ids", 5, 2, seed=(0xDEADBEEF << 32) | 420),
] + [_pcase(f"params.rrc-{hw[0]}x{hw[1]}", "params.rrc", 96, 2, hw, _cfg(scale_min=s[0], scale_max=s[1])) for hw, s, _ in RRC_SOURCES] + [
    _pcase("params.cfg-zero", "params.cfg", 40, 2, cfg=_cfg(brightness=0.0, contrast=0.0, saturation=0.0, hue=0.0)),
    _pcase("params.cfg-p0", "params.cfg", 40, 2, cfg=_cfg(p_jitter=0.0, p_gray=0.0, p_flip=0.0)),
    _pcase("params.cfg-p1", "params.cfg", 40, 2, cfg=_cfg(p_jitter=1.0, p_gray=1.0, p_flip=1.0)),
    _pcase("params.cfg-bright", "params.cfg", 40, 2, cfg=_cfg(brightness=1.5)),
    _pcase("params.cfg-scale", "params.cfg", 40, 2, cfg=_cfg(scale_min=0.5, scale_max=0.5)),
    _pcase("params.cfg-ratio", "params.cfg", 40, 2, cfg=_cfg(ratio_min=1.0, ratio_max=1.0)),
] + [_pcase(f"params.blur-{b}x{v}", "params.blur", b, v, blur=(0.5, 0.1, 2.0)) for b, v in TAILS] + [
    _pcase("params.blur-p0", "params.blur", 40, 2, blur=(0.0, 0.1, 2.0)),
    _pcase("params.blur-p1", "params.blur", 40, 2, blur=(1.0, 0.1, 2.0)),
    _pcase("params.blur-sigma", "params.blur", 40, 2, blur=(0.5, 1.5, 1.5)),
]


def param_records(pc):
    """(records float32 [V, B, 16], branches [V][B], smallest margin) of a parameter case"""
    out = [[draw_record(pc["seed"], pc["step"], pc["ids"][k] if pc["ids"] is not None else pc["sample0"] + k, v, pc["hs"], pc["ws"], pc["cfg"], pc["blur"])
            for k in range(pc["B"])] for v in range(pc["V"])]
    return np.stack([np.stack([r[0] for r in row]) for row in out]), [[r[1] for r in row] for row in out], min(r[2] for row in out for r in row)


def _bcase(cid, label, b, ncrop, base=16, hw=(32, 32), scale=(0.3, 1.0), ids=None, sample0=0):
    return dict(id=cid, label=label, B=b, ncrop=ncrop, view_base=base, hs=hw[0], ws=hw[1], scale=scale, seed=SEED, step=STEP,
                ids=None if ids is None else [int(i) for i in ids], sample0=sample0)


BOX_CASES = [_bcase(f"boxes.tail-{b}x{n}", "boxes.tail", b, n) for b, n in ((1, 1), (9, 7), (8, 8), (13, 5))] + [
    _bcase("boxes.base-144", "boxes.base", 7, 6, 144, scale=(0.08, 0.3)), _bcase("boxes.base-400", "boxes.base", 7, 6, 400, scale=(0.08, 0.3)),
    _bcase("boxes.base-65535", "boxes.base", 7, 1, 65535),
] + [_bcase(f"boxes.rrc-{hw[0]}x{hw[1]}", "boxes.rrc", 24, 4, hw=hw, scale=s) for hw, s, _ in RRC_SOURCES] + [
    _bcase("boxes.ids-sample0", "boxes.ids", 6, 3, sample0=1000), _bcase("boxes.ids-explicit", "boxes.ids", 6, 3, ids=1000 + np.arange(6)),
    _bcase("boxes.ids-big", "boxes.ids", 3, 2, ids=BIG_IDS)]


def box_records(bc):
    """(boxes int32 [B, ncrop, 4], branches, smallest margin) of a box case"""
    out = [[draw_boxes(bc["seed"], bc["step"], bc["ids"][k] if bc["ids"] is not None else bc["sample0"] + k, bc["view_base"], c, bc["hs"], bc["ws"], bc["scale"])
            for c in range(bc["ncrop"])] for k in range(bc["B"])]
    return np.array([[r[0] for r in row] for row in out], np.int32), [[r[1] for r in row] for row in out], min(r[2] for row in out for r in row)


# ------------------------------------------------------------------------------------------- refusals
# An accepted call per entry point (BASES) and one changed argument per refusal.  Pointer arguments are named; None is a null pointer.  `src_hw` of a call is what
# its source buffer is allocated for (the 4096 x 4096 source is allocated for real).
BASES = {
    "ssv_augment_params": dict(B=5, Hs=40, Ws=36, nviews=2, cfg=dict(DEFAULT_CFG), seed=SEED, step=STEP, ids=None, sample0=0, params=True),
    "ssv_augment_params_blur": dict(B=5, Hs=40, Ws=36, nviews=2, cfg=dict(DEFAULT_CFG), seed=SEED, step=STEP, ids=None, sample0=0, p_blur=0.5, sigma_min=0.1,
                                    sigma_max=2.0, params=True),
    "ssv_augment_views": dict(B=2, nviews=2, Hs=96, Ws=40, Ho=32, Wo=32, src=True, ids=None, params=True, mean=True, std=True, out=True, ws=True, short=0),
    "ssv_augment_views_blur": dict(B=2, nviews=2, Hs=96, Ws=40, Ho=32, Wo=32, src=True, ids=None, params=True, mean=True, std=True, out=True, ws=True, short=0),
    "ssv_center_view": dict(B=2, Hs=9, Ws=8, Ho=6, Wo=6, src=True, ids=None, mean=True, std=True, out=True),
    "ssv_multicrop_params": dict(B=4, Hs=32, Ws=32, ncrop=3, view_base=16, scale_min=0.3, scale_max=1.0, seed=SEED, step=STEP, ids=None, sample0=0, boxes=True),
}
WIDE_BASE = dict(Hs=8, Ws=4096, Ho=4, Wo=1366)                             # accepted; Hs = 4096 alone then makes Hs * Ws = 2^24


def _refusals():
    out = []
    add = lambda label, entry, what, change, rc=ERR_INVALID, base=None: out.append(dict(id=f"{label}-{entry[4:]}-{what}", label=label, entry=entry, change=change, rc=rc,
                                                                                          base=base or {}))
    for e in ("ssv_augment_params", "ssv_augment_params_blur"):
        for k in ("B", "Hs", "Ws", "nviews"):
            add("refuse.params", e, f"{k}=0", {k: 0})
            add("refuse.params", e, f"{k}=-1", {k: -1})
        add("refuse.params", e, "nviews=17", {"nviews": 17})
        add("refuse.params", e, "cfg=null", {"cfg": None})
        add("refuse.params", e, "params=null", {"params": None})
        for what, cfg in (("scale_min=0", _cfg(scale_min=0.0)), ("scale_max<min", _cfg(scale_min=0.5, scale_max=0.4)), ("ratio_min=0", _cfg(ratio_min=0.0)),
                          ("ratio_max<min", _cfg(ratio_min=1.0, ratio_max=0.9)), ("scale_min=-1", _cfg(scale_min=-1.0))):
            add("refuse.params", e, what, {"cfg": cfg})
    e = "ssv_augment_params_blur"
    for what, change in (("p_blur=-0.1", {"p_blur": -0.1}), ("p_blur=1.1", {"p_blur": 1.1}), ("p_blur=nan", {"p_blur": float("nan")}), ("sigma_min=-1", {"sigma_min": -1.0}),
                         ("sigma_max<min", {"sigma_max": 0.05}), ("sigma_max=1000.5", {"sigma_max": BLUR_MAX_SIGMA + 0.5}), ("sigma=nan", {"sigma_max": float("nan")})):
        add("refuse.params", e, what, change)
    for e, label in (("ssv_augment_views", "refuse.views"), ("ssv_augment_views_blur", "refuse.blur")):
        for k in ("B", "nviews", "Hs", "Ws", "Ho", "Wo"):
            add(label, e, f"{k}=0", {k: 0})
            add(label, e, f"{k}=-1", {k: -1})
        for k in ("src", "params", "mean", "std", "out", "ws"):
            add(label, e, f"{k}=null", {k: None})
        add(label, e, "Hs=97", {"Hs": 97})                                 # 96 -> 32 is accepted (the base call), 97 -> 32 needs a ninth tap
        add(label, e, "Ws=97", {"Ws": 97})
        add(label, e, "Hs=4096", {"Hs": 4096}, base=WIDE_BASE)
        add("refuse.workspace", e, "short", {"short": 1}, ERR_WORKSPACE)
        add("refuse.workspace", e, "ws_bytes=0", {"short": -1}, ERR_WORKSPACE)                   # short = -1: ws_bytes 0 with a real buffer
    add("refuse.blur", "ssv_augment_views_blur", "141x581", {"Wo": 581}, base=dict(Ho=141, Wo=580))             # 141 * 581 = 81921 = SSV_BLUR_MAX_PIXELS + 1
    add("refuse.blur", "ssv_augment_views_blur", "1x81921", {"Wo": 81921}, base=dict(Hs=3, Ho=1, Wo=81920))
    add("refuse.blur", "ssv_augment_views_blur", "B=2^30", {"B": 1 << 30})                       # 3 * nviews * B workgroups no longer fit an int
    add("refuse.blur", "ssv_augment_views_blur", "ws+4", {"ws": "misaligned"})                   # the staging image behind the tables must stay 16-byte aligned
    e = "ssv_center_view"
    for k in ("B", "Ho", "Wo"):
        add("refuse.center", e, f"{k}=0", {k: 0})
        add("refuse.center", e, f"{k}=-1", {k: -1})
    for what, change in (("Ho>Hs", {"Ho": 10}), ("Wo>Ws", {"Wo": 9}), ("Hs=0", {"Hs": 0}), ("Ws=-1", {"Ws": -1})):
        add("refuse.center", e, what, change)
    for k in ("src", "mean", "std", "out"):
        add("refuse.center", e, f"{k}=null", {k: None})
    e = "ssv_multicrop_params"
    for k in ("B", "Hs", "Ws", "ncrop"):
        add("refuse.boxes", e, f"{k}=0", {k: 0})
        add("refuse.boxes", e, f"{k}=-1", {k: -1})
    for what, change in (("view_base=15", {"view_base": 15}), ("view_base+ncrop=65537", {"view_base": 65534}), ("boxes=null", {"boxes": None}),
                         ("scale_min=0", {"scale_min": 0.0}), ("scale_max<min", {"scale_max": 0.2}), ("scale=nan", {"scale_min": float("nan")})):
        add("refuse.boxes", e, what, change)
    return out


REFUSALS = _refusals()
WORKSPACE_REFUSALS = [(0, 2, 8, 8), (2, 0, 8, 8), (2, 2, 0, 8), (2, 2, 8, 0), (-1, 2, 8, 8), (2, 2, 8, -3)]      # both *_workspace_bytes return 0
BLUR_WORKSPACE_REFUSALS = [(2, 2, 141, 581), (1, 1, 1, 81921), (1, 1, 321, 256)]                                  # ... and the blur one above SSV_BLUR_MAX_PIXELS


def call_of(r):
    """the arguments of a refusal: the entry point's accepted call, the refusal's own base on top, then its one change"""
    return dict(BASES[r["entry"]], **r["base"]), dict(BASES[r["entry"]], **dict(r["base"], **r["change"]))


def verdict(entry, a):
    """the return code the SSV_REQUIREs of `entry` give the call `a`, restated (a workspace `short` of the library's own size gives SSV_ERR_WORKSPACE)"""
    pos = lambda *ks: all(a[k] > 0 for k in ks)
    ptrs = lambda *ks: all(a[k] is not None for k in ks)
    if entry in ("ssv_augment_params", "ssv_augment_params_blur"):
        if not (pos("B", "Hs", "Ws", "nviews") and a["nviews"] <= 16 and ptrs("cfg", "params")):
            return ERR_INVALID
        if entry.endswith("blur") and not (0.0 <= a["p_blur"] <= 1.0 and a["sigma_min"] >= 0.0 and a["sigma_min"] <= a["sigma_max"] <= BLUR_MAX_SIGMA):
            return ERR_INVALID
        c = a["cfg"]
        return OK if c["scale_min"] > 0 and c["scale_max"] >= c["scale_min"] and c["ratio_min"] > 0 and c["ratio_max"] >= c["ratio_min"] else ERR_INVALID
    if entry in ("ssv_augment_views", "ssv_augment_views_blur"):
        if not (pos("B", "nviews", "Hs", "Ws", "Ho", "Wo") and ptrs("src", "params", "mean", "std", "out", "ws")):
            return ERR_INVALID
        if not (a["Hs"] * a["Ws"] < MAX_SOURCE_PIXELS and accepted(a["Hs"], a["Ho"]) and accepted(a["Ws"], a["Wo"])):
            return ERR_INVALID
        if entry.endswith("blur") and (a["Ho"] * a["Wo"] > BLUR_MAX_PIXELS or a["nviews"] * a["B"] > (2 ** 31 - 1) // 3):
            return ERR_INVALID
        if a["short"]:
            return ERR_WORKSPACE
        return ERR_INVALID if a["ws"] == "misaligned" else OK
    if entry == "ssv_center_view":
        return OK if pos("B", "Ho", "Wo") and a["Hs"] >= a["Ho"] and a["Ws"] >= a["Wo"] and ptrs("src", "mean", "std", "out") else ERR_INVALID
    assert entry == "ssv_multicrop_params"
    ok = pos("B", "Hs", "Ws", "ncrop") and a["view_base"] >= 16 and a["view_base"] + a["ncrop"] <= 65536 and ptrs("boxes")
    return OK if ok and a["scale_min"] > 0 and a["scale_max"] >= a["scale_min"] else ERR_INVALID


def marshal(entry, a, ptr, stream):
    """the ctypes argument list of the call `a`: ptr(name) -> the address of that buffer (asked only for non-null pointers), `ws_bytes` from ptr("ws_bytes")"""
    import ctypes as C
    from ssv_amd import _lib
    P = lambda k: None if a[k] is None else ptr(k) + (4 if a[k] == "misaligned" else 0)
    ids = None if a.get("ids") is None else ptr("ids")
    cfg = lambda: None if a["cfg"] is None else C.byref(_lib.AugCfg(*[float(a["cfg"][k]) for k in CFG_FIELDS]))
    f3 = lambda k: None if a[k] is None else C.cast(ptr(k), C.POINTER(C.c_float))
    if entry == "ssv_augment_params":
        return [a["B"], a["Hs"], a["Ws"], a["nviews"], cfg(), a["seed"], a["step"], ids, a["sample0"], P("params"), stream]
    if entry == "ssv_augment_params_blur":
        return [a["B"], a["Hs"], a["Ws"], a["nviews"], cfg(), a["seed"], a["step"], ids, a["sample0"], a["p_blur"], a["sigma_min"], a["sigma_max"], P("params"), stream]
    if entry in ("ssv_augment_views", "ssv_augment_views_blur"):
        full = ptr("ws_bytes")
        nbytes = 0 if a["short"] < 0 else full - a["short"]
        return [a["B"], a["nviews"], a["Hs"], a["Ws"], a["Ho"], a["Wo"], P("src"), ids, P("params"), f3("mean"), f3("std"), P("out"), P("ws"), nbytes, stream]
    if entry == "ssv_center_view":
        return [a["B"], a["Hs"], a["Ws"], a["Ho"], a["Wo"], P("src"), ids, f3("mean"), f3("std"), P("out"), stream]
    assert entry == "ssv_multicrop_params"
    return [a["B"], a["Hs"], a["Ws"], a["ncrop"], a["view_base"], a["scale_min"], a["scale_max"], a["seed"], a["step"], ids, a["sample0"], P("boxes"), stream]


# ------------------------------------------------------------------------------------------- the front-end pass
FRONT_DROPS = (None, "color_jitter", "random_gray", "random_flip")
MULTICROP = dict(num_local_views=3, num_global_views=2, global_size=[6, 6], local_size=[4, 4], scale_threshold=0.3)


def front_chain(size, drop=None):
    """the YAML transform block of the two-view chain, one optional transform dropped"""
    c = {"color_jitter": {"brightness": 0.4, "contrast": 0.4, "saturation": 0.4, "hue": 0.1, "apply_prob": 0.8}, "random_gray": {"p": 0.2},
         "random_resized_crop": {"size": list(size), "scale": [0.2, 1.0]}, "random_flip": None, "to_tensor": None, "normalize": {"mean": MEAN, "std": STD}}
    if drop:
        del c[drop]
    return c


def front_cfg(drop=None):
    """what dropping that transform means to the draws: its probability is 0 (and a dropped jitter has no strengths); the stream is consumed all the same"""
    return dict(DEFAULT_CFG, **{None: {}, "color_jitter": dict(brightness=0.0, contrast=0.0, saturation=0.0, hue=0.0, p_jitter=0.0), "random_gray": dict(p_gray=0.0),
                                "random_flip": dict(p_flip=0.0)}[drop])


def front_records(ids, hs, ws, drop=None, nviews=2):
    """(records [V, B, 16], smallest margin) GpuTransform.draw must give for the chain front_chain(.., drop)"""
    out = [[draw_record(SEED, STEP, int(i), v, hs, ws, front_cfg(drop)) for i in ids] for v in range(nviews)]
    return np.stack([np.stack([r[0] for r in row]) for row in out]), min(r[2] for row in out for r in row)


def front_boxes(ids, hs, ws, copy, kind):
    """(boxes int32 [B, ncrop, 4], smallest margin) of MultiCrop.__call__ for one copy: global crops on views 16 + 256 copy .., local ones on 144 + 256 copy .."""
    ncrop, scale, base = {"global": (MULTICROP["num_global_views"], (MULTICROP["scale_threshold"], 1.0), 16),
                          "local": (MULTICROP["num_local_views"], (0.08, MULTICROP["scale_threshold"]), 144)}[kind]
    out = [[draw_boxes(SEED, STEP, int(i), base + 256 * copy, c, hs, ws, scale) for c in range(ncrop)] for i in ids]
    return np.array([[r[0] for r in row] for row in out], np.int32), min(r[2] for row in out for r in row)
