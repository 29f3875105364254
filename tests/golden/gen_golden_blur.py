#!/usr/bin/env python3
"""Generate tests/golden/blur_level.npz with THE INSTALLED PILLOW (Image.filter(ImageFilter.GaussianBlur(radius=sigma))):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_blur.py

The inputs are the seeded 5 x 4 and 33 x 17 RGB images of tests/blur_oracle.py (the tests regenerate them; they are not stored) and the sigmas are
its fixed list.  tests/test_blur_cpu.py holds the numpy restatement both to this file and to the Pillow that is installed when it runs, so a Pillow
release that changes BoxBlur.c shows up as a disagreement between the two and not as a silent drift.  The archive is written with fixed zip
timestamps: regenerating it with the same Pillow gives the same bytes.
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import blur_oracle as bo           # noqa: E402

SHAPES = ((5, 4), (33, 17))


def write_npz(path, arrays):
    """np.savez_compressed with constant member timestamps."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def main():
    import PIL
    out = {"sigmas": np.asarray(bo.SIGMAS, np.float32), "pillow_version": np.frombuffer(PIL.__version__.encode(), np.uint8)}
    for h, w in SHAPES:
        img = bo.seeded_image(h, w)
        out[f"blur_{h}x{w}"] = np.stack([bo.gaussian_blur_pil(img, s) for s in out["sigmas"]])
    write_npz(os.path.join(HERE, "blur_level.npz"), out)
    print("blur_level: Pillow", PIL.__version__, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
