"""GPU: gaussian_blur in the fused augmentation chain against the Pillow-pinned restatement (tests/blur_oracle.py).  Everything is integer arithmetic up to
the final ToTensor / Normalize, whose three float32 operations are the unblurred chain's: all comparisons are exact."""
import numpy as np
import pytest
import torch

import blur_oracle as bo
from oracle import augment as A

pytestmark = pytest.mark.gpu
MEAN, STD = [0.4914, 0.4822, 0.4465], [0.2470, 0.2435, 0.2616]
SEED, STEP = 420, 7                                  # GpuTransform's default seed; the draws below are checked on the CPU for exactly this pair


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _cfg(size, blur=None):
    c = {"color_jitter": {"brightness": 0.4, "contrast": 0.4, "saturation": 0.4, "hue": 0.1, "apply_prob": 0.8}, "random_gray": {"p": 0.2},
         "random_resized_crop": {"size": list(size), "scale": [0.2, 1.0]}, "random_flip": None}
    if blur is not None:
        c["gaussian_blur"] = blur
    c.update({"to_tensor": None, "normalize": {"mean": MEAN, "std": STD}})
    return c


def test_draws_keep_the_record_and_add_the_blur_slot(dev):
    from ssv_amd.utils import augmentations
    b, hw, lo, hi = 64, (40, 36), 0.1, 2.0
    imgs = torch.zeros((b + 9, hw[0], hw[1], 3), dtype=torch.uint8, device=dev)
    idx = torch.tensor(np.random.default_rng(1).permutation(b + 9)[:b].astype(np.int64))
    ref = np.stack([[A.draw_params(SEED, STEP, int(i), v, hw[0], hw[1]) for i in idx] for v in range(2)])
    plain = augmentations.get_transform(_cfg((32, 32))).draw(imgs, idx.to(dev), step=STEP).cpu().numpy()
    np.testing.assert_array_equal(plain, ref)
    for p in (0.5, 0.0, 1.0):
        want15 = np.array([[bo.draw_blur(SEED, STEP, int(i), v, p, lo, hi) for i in idx] for v in range(2)], np.float32)
        on = int((want15 > 0).sum())
        assert {0.5: 8 <= on <= 120, 0.0: on == 0, 1.0: on == 128}[p], on               # the restatement's draws for this seed: both branches are taken
        got = augmentations.get_transform(_cfg((32, 32), {"sigma": [lo, hi], "apply_prob": p})).draw(imgs, idx.to(dev), step=STEP).cpu().numpy()
        np.testing.assert_array_equal(got[..., :15], ref[..., :15])
        np.testing.assert_array_equal(got[..., 15], want15)


def test_scalars_equal_the_restatement(dev):
    from ssv_amd import _lib
    sig = np.concatenate([np.asarray(bo.SIGMAS, np.float32), bo.seeded_sigmas(), np.float32([0.0, 1e-4, 1e-3, 0.02])])       # 0: box radius 0, Pillow copies
    out = torch.full((sig.size, 3), -7, dtype=torch.int32, device=dev)
    _lib.call("ssv_blur_scalars", sig.size, _lib.ptr(torch.from_numpy(sig).to(dev)), _lib.ptr(out), _lib.stream())
    want = np.array([bo.scalars(s) or (-1, 0, 0) for s in sig], np.int64)
    assert (want[:len(bo.SIGMAS) + 200, 0] >= 0).all()
    np.testing.assert_array_equal(out.cpu().numpy(), want)


# source, output, B, sigma per (view, sample): 0 = that record is not blurred
CASES = [((40, 36), (32, 32), 3, [[0.1, 0.3, 2.0], [0.0, 2.0, 0.0]]),
         ((40, 36), (24, 40), 3, [[3.7, 0.0, 3.7], [3.7, 3.7, 0.0]]),         # not square: a transposed pass shows
         ((12, 12), (5, 4), 2, [[8.0, 25.0], [0.0, 8.0]]),                    # radius >= size in both directions
         ((256, 240), (224, 224), 2, [[2.0, 2.0], [0.0, 2.0]]),               # the largest LDS class
         ((260, 258), (256, 256), 1, [[1.0], [0.0]])]                         # Ho * Wo = 65536: the size the layout has to hold


@pytest.mark.parametrize("src_hw,out_hw,b,sigmas", CASES)
def test_pixels_bit_exact_vs_pillow_restatement(dev, src_hw, out_hw, b, sigmas):
    from ssv_amd.utils import augmentations
    rng = np.random.default_rng(5)
    imgs = rng.integers(0, 256, (b + 2, src_hw[0], src_hw[1], 3), dtype=np.uint8)
    imgs[1] = (imgs[1] // 85) * 85                                        # few levels
    idx = torch.tensor(rng.permutation(b + 2)[:b].astype(np.int64))
    tf = augmentations.get_transform(_cfg(out_hw, {"sigma": [0.1, 2.0], "apply_prob": 0.5}))
    d_imgs, d_idx = torch.from_numpy(imgs).to(dev), idx.to(dev)
    p = tf.draw(d_imgs, d_idx, step=STEP).cpu().numpy().copy()
    p[..., 15] = np.asarray(sigmas, np.float32)
    p[0, 0, 0], p[0, 0, 1:5], p[0, 0, 14] = 1, [3, 1, 0, 2], 1           # the first record: jitter, flip and blur together
    p[1, min(1, b - 1), 10:14] = [0, 0, src_hw[0], src_hw[1]]                         # whole image: the down-scaling path in front of the blur
    assert p[0, 0, 15] > 0 and (p[..., 15] == 0).any()
    out = tf.apply(d_imgs, d_idx, torch.from_numpy(p).to(dev)).cpu().numpy()
    assert out.shape == (2, b, 3, out_hw[0], out_hw[1])
    for v in range(2):
        for k in range(b):
            ref = bo.view_numpy_blur(imgs[int(idx[k])], p[v, k], out_hw, MEAN, STD)
            np.testing.assert_array_equal(out[v, k], ref, err_msg=f"view {v} sample {k} params {p[v, k]}")
    np.testing.assert_array_equal(out[0, 0], bo.view_pil_blur(imgs[int(idx[0])], p[0, 0], out_hw, MEAN, STD))
    if out_hw == (32, 32):                                                # unblurred records: the bits of the chain without blur
        plain = augmentations.get_transform(_cfg(out_hw)).apply(d_imgs, d_idx, torch.from_numpy(p).to(dev)).cpu().numpy()
        off = p[..., 15] == 0
        np.testing.assert_array_equal(out[off], plain[off])
        assert not np.array_equal(out[~off], plain[~off])


def test_multicrop_and_loader_get_blur_through_draw_and_apply(dev):
    from ssv_amd.utils import augmentations, data_utils
    rng = np.random.default_rng(8)
    imgs = rng.integers(0, 256, (8, 40, 36, 3), dtype=np.uint8)
    blur = {"sigma": [0.1, 2.0], "apply_prob": 0.5}
    mc = augmentations.MultiCrop({"num_local_views": 3, "num_global_views": 2, "global_size": [32, 32], "local_size": [16, 16], "scale_threshold": 0.3,
                                  "train_transforms": _cfg((32, 32), blur)})
    d_imgs, idx = torch.from_numpy(imgs).to(dev), torch.arange(8, device=dev)
    crops = mc(d_imgs, idx, STEP)
    for k, shape in (("global_1", (8, 2, 3, 32, 32)), ("global_2", (8, 2, 3, 32, 32)), ("local_1", (8, 3, 3, 16, 16)), ("local_2", (8, 3, 3, 16, 16))):
        assert crops[k].shape == shape and torch.isfinite(crops[k]).all(), k
    p = mc.transforms.draw(d_imgs, idx, STEP, 2)
    views = mc.transforms.apply(d_imgs, idx, p).cpu().numpy()
    p = p.cpu().numpy()
    v, k = np.argwhere(p[..., 15] > 0)[0]
    assert p[v, k, 15] == bo.draw_blur(SEED, STEP, int(k), int(v), 0.5, 0.1, 2.0)
    np.testing.assert_array_equal(views[v, k], bo.view_numpy_blur(imgs[k], p[v, k], (32, 32), MEAN, STD))
    # the two-view loader: apply_prob 0 gives the plain chain's batches bit for bit, apply_prob 1 blurs every view
    test_tf = {"center_crop": {"size": [32, 32]}, "to_tensor": None, "normalize": {"mean": MEAN, "std": STD}}
    first = {}
    for name, chain in (("plain", _cfg((32, 32))), ("p0", _cfg((32, 32), {"apply_prob": 0.0})), ("p1", _cfg((32, 32), {"sigma": [1.0, 2.0]}))):
        loader = data_utils.GpuTwoViewLoader(imgs, np.arange(8) % 3, {"train": chain, "test": test_tf}, batch_size=4, shuffle=False, device=dev)
        first[name] = next(iter(loader))
    for key in ("aug_1", "aug_2"):
        assert torch.equal(first["p0"][key], first["plain"][key])
        assert (first["p1"][key] != first["plain"][key]).flatten(1).any(1).all()


def test_output_above_the_lds_layout_is_refused(dev):
    from ssv_amd import _lib
    from ssv_amd.utils import augmentations
    assert 288 * 288 > _lib.BLUR_MAX_PIXELS >= 65536
    imgs = torch.zeros((1, 300, 300, 3), dtype=torch.uint8, device=dev)
    idx = torch.zeros(1, dtype=torch.int64, device=dev)
    tf = augmentations.get_transform(_cfg((288, 288), {"sigma": [0.1, 2.0], "apply_prob": 0.5}))
    with pytest.raises(_lib.SsvError, match="LDS"):
        tf.apply(imgs, idx, tf.draw(imgs, idx, step=0))
    out = augmentations.get_transform(_cfg((288, 288))).apply(imgs, idx, tf.draw(imgs, idx, step=0))      # the chain without blur has no such limit
    assert out.shape == (2, 1, 3, 288, 288)
