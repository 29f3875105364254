"""TEST INFRASTRUCTURE - CPU restatement (numpy) of Pillow's ImageFilter.GaussianBlur (BoxBlur.c) and of the blur draws of the GPU augmentation
chain, in the style of oracle/augment.py, pinned to the installed Pillow and to tests/golden/blur_level.npz by tests/test_blur_cpu.py.

Pillow's Gaussian blur is three passes of an "extended box blur" (Gwosdek et al., SSVM 2011) along the rows, then three along the columns, in 32-bit
fixed point with a uint8 image between the passes:
  * `box_radius`   the fractional box radius of a standard deviation; float32 arithmetic except where C promotes to double (the widths matter: sigma
                   = 0.3 gives another radius when the divisor is evaluated in double);
  * `scalars`      (radius, ww, fw): the integer radius, the weight of a pixel inside the box and the weight of the two pixels at its fractional edge;
  * `line_pass`    one pass along the last axis; the closed form of Pillow's sliding accumulator, edge pixels repeated (also when radius >= n);
  * `gaussian_blur` the six passes of an [H, W, C] uint8 image.
`draw_blur` is slot [15] of the parameter record: the blur draws come from a Philox stream of their own, keyed (seed, step, sample, 1024 + view), so
slots [0..14] stay what oracle.augment.draw_params gives.  `view_pil_blur` / `view_numpy_blur` are oracle.augment.view_pil / view_numpy with the blur
between the flip and ToTensor (oracle/ does not expose its uint8 stage, so those few lines are restated here).
"""
import math

import numpy as np

from oracle import augment as A

SIGMAS = (0.1, 0.29, 0.3, 0.31, 0.5, 1.0, 2.0, 3.7, 8.0, 25.0)        # radius 0, fractional-only weights, the float-evaluation case, radius >= width
BLUR_VIEW_BASE = 1024                                                  # the two-view streams use views 0..15, MultiCrop's boxes up to ~420


def seeded_sigmas(n=200, lo=0.1, hi=2.0, seed=11):
    return np.random.default_rng(seed).uniform(lo, hi, n).astype(np.float32)


def seeded_image(h, w, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ------------------------------------------------------------------------------------------- the restatement
def box_radius(sigma):
    """BoxBlur.c _gaussian_blur_radius(sigma, passes = 3) -> float32."""
    f32 = np.float32
    sigma = f32(sigma)
    s2 = f32(f32(sigma * sigma) / f32(3))
    L = f32(math.sqrt(12.0 * float(s2) + 1.0))
    l = f32(math.floor((float(L) - 1.0) / 2.0))
    a = f32(float(f32(2) * l + f32(1)) * (float(l * (l + f32(1))) - 3.0 * float(s2)))
    lp1 = f32(l + f32(1))
    a = f32(a / f32(f32(6) * f32(s2 - f32(lp1 * lp1))))
    return f32(l + a)


def scalars(sigma):
    """(radius, ww, fw) of ImagingLineBoxBlur8 for the box radius of `sigma`; None where Pillow copies (box radius 0)."""
    fr = box_radius(sigma)
    if fr == 0:
        return None
    radius = int(fr)
    ww = int(np.float32(1 << 24) / np.float32(fr * np.float32(2) + np.float32(1)))
    fw = ((1 << 24) - (2 * radius + 1) * ww) // 2
    return radius, ww, fw


def line_pass(img, radius, ww, fw):
    """One extended-box pass along the LAST axis of a uint8 array."""
    n = img.shape[-1]
    x = img.astype(np.int64)
    pos = np.arange(n)
    acc = np.zeros_like(x)
    for d in range(-radius, radius + 1):
        acc += x[..., np.clip(pos + d, 0, n - 1)]
    edge = x[..., np.clip(pos - radius - 1, 0, n - 1)] + x[..., np.clip(pos + radius + 1, 0, n - 1)]
    out = (ww * acc + fw * edge + (1 << 23)) & 0xFFFFFFFF                       # uint32 arithmetic (it never wraps: the weights sum to <= 2^24)
    return (out >> 24).astype(np.uint8)


def gaussian_blur(img_u8, sigma):
    """Image.filter(ImageFilter.GaussianBlur(radius=sigma)) of an [H, W, C] (or [H, W]) uint8 image."""
    sc = scalars(sigma) if sigma > 0 else None
    if sc is None:
        return img_u8.copy()
    x = np.moveaxis(img_u8, 1, -1)                           # rows: W last
    for _ in range(3):
        x = line_pass(x, *sc)
    x = np.moveaxis(np.moveaxis(x, -1, 1), 0, -1)            # columns: H last
    for _ in range(3):
        x = line_pass(x, *sc)
    return np.ascontiguousarray(np.moveaxis(x, -1, 0))


def gaussian_blur_pil(img_u8, sigma):
    from PIL import Image, ImageFilter
    mode = "RGB" if img_u8.ndim == 3 else "L"
    return np.asarray(Image.fromarray(np.ascontiguousarray(img_u8), mode).filter(ImageFilter.GaussianBlur(radius=float(sigma))), dtype=np.uint8)


# ------------------------------------------------------------------------------------------- the draws
def draw_blur(seed, step, sample, view, p, lo, hi):
    """Slot [15]: the drawn sigma as float32, 0 = no blur.  u0 decides (apply iff u0 < p); u1 is drawn either way."""
    st = A._Stream(seed, step, sample, BLUR_VIEW_BASE + view)
    u0, u1 = st.uniform(), st.uniform()
    sigma = np.float32(lo + u1 * (hi - lo))
    return sigma if u0 < p else np.float32(0)


# ------------------------------------------------------------------------------------------- the chain with blur
def _normalise(img, mean, std):
    t = img.astype(np.float32) / np.float32(255)
    t = (t - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)
    return np.ascontiguousarray(t.transpose(2, 0, 1))


def view_u8_numpy(img_u8, p, out_hw):
    """The uint8 image oracle.augment.view_numpy holds in front of ToTensor."""
    img = A.color_ops_numpy(np.ascontiguousarray(img_u8), p)
    top, left, ch, cw = int(p[10]), int(p[11]), int(p[12]), int(p[13])
    img = A.resize_bilinear_numpy(img[top:top + ch, left:left + cw], out_hw)
    return img[:, ::-1] if p[14] >= 0.5 else img


def view_numpy_blur(img_u8, p, out_hw, mean, std):
    img = np.ascontiguousarray(view_u8_numpy(img_u8, p, out_hw))
    if p[15] > 0:
        img = gaussian_blur(img, np.float32(p[15]))
    return _normalise(img, mean, std)


def view_pil_blur(img_u8, p, out_hw, mean, std):
    """oracle.augment.view_pil's recipe with ImageFilter.GaussianBlur between the flip and ToTensor."""
    from PIL import Image, ImageEnhance, ImageFilter
    img = Image.fromarray(np.ascontiguousarray(img_u8), "RGB")
    if p[0] >= 0.5:
        for op in (int(p[1]), int(p[2]), int(p[3]), int(p[4])):
            if op == 0:
                img = ImageEnhance.Brightness(img).enhance(float(np.float32(p[5])))
            elif op == 1:
                img = ImageEnhance.Contrast(img).enhance(float(np.float32(p[6])))
            elif op == 2:
                img = ImageEnhance.Color(img).enhance(float(np.float32(p[7])))
            else:
                h, s, v = img.convert("HSV").split()
                shift = int(float(np.float32(p[8])) * 255) % 256
                nh = (np.array(h, dtype=np.uint8).astype(np.int32) + shift) % 256
                img = Image.merge("HSV", (Image.fromarray(nh.astype(np.uint8), "L"), s, v)).convert("RGB")
    if p[9] >= 0.5:
        g = img.convert("L")
        img = Image.merge("RGB", (g, g, g))
    top, left, ch, cw = int(p[10]), int(p[11]), int(p[12]), int(p[13])
    img = img.crop((left, top, left + cw, top + ch)).resize((out_hw[1], out_hw[0]), Image.BILINEAR)
    if p[14] >= 0.5:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    if p[15] > 0:
        img = img.filter(ImageFilter.GaussianBlur(radius=float(np.float32(p[15]))))
    return _normalise(np.asarray(img, dtype=np.uint8), mean, std)
