"""Writes tests/golden/drivable_pil.npz: the seeded lane maps of tests/drivable_cases.py (PIL_CASES) drawn by Pillow's ImageDraw.polygon
with fill and outline -- a scanline rasteriser that is not ours, standing in for cv2.fillPoly, which is not installed.  Per case: the polygons
(vertices + poly_start), the pose, H, W, res and the mask (1 = off road).  Pillow gets the rounded pixel vertices of the rule, as
cv2.fillPoly gets them in the reference (traj_evaluator.py:329-331).

    python tests/golden/gen_drivable.py
"""
import os
import sys

import numpy as np
from PIL import Image, ImageDraw

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import drivable_cases as D      # noqa: E402


def main():
    out = {"n_case": np.int64(len(D.PIL_CASES))}
    for i, (seed, H, W, res) in enumerate(D.PIL_CASES):
        polys, pose = D.pil_case(seed, H, W, res)
        img = Image.new("L", (W, H), 1)
        draw = ImageDraw.Draw(img)
        for p in polys:
            v = D.rounded_vertices(p, pose, res, H, W)
            draw.polygon([(int(x), int(y)) for x, y in v], fill=0, outline=0)
        out[f"{i}.vertices"] = np.concatenate(polys, 0)
        out[f"{i}.poly_start"] = np.concatenate([[0], np.cumsum([len(p) for p in polys])]).astype(np.int32)
        out[f"{i}.n_polys"] = np.int64(len(polys))
        out[f"{i}.pose"] = np.asarray(pose, dtype=np.float64)
        out[f"{i}.H"], out[f"{i}.W"], out[f"{i}.res"] = np.int64(H), np.int64(W), np.float64(res)
        out[f"{i}.mask"] = np.asarray(img, dtype=np.uint8)
    path = os.path.join(HERE, "drivable_pil.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
