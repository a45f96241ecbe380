"""tools/validate_real.py on a directory of PNGs: the files it takes and the pixels it writes."""
import json
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from perseus_amd.detector import denormalize_pixel_coordinates

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tool_writes_forward_real_pixels(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import validate_real
    finally:
        sys.path.pop(0)
    rng = np.random.default_rng(0)
    imgs = {"img_0.png": (256, 256), "img_1.png": (300, 400), "img_1_segmentation.png": (300, 400)}
    data = {}
    for name, (h, w) in imgs.items():
        data[name] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        Image.fromarray(data[name]).save(tmp_path / name)
    out = tmp_path / "kp.json"
    validate_real.main([str(tmp_path), "--out", str(out)])
    got = json.loads(out.read_text())
    assert sorted(got) == ["img_0.png", "img_1.png"]
    m = validate_real.load_model()
    for name in got:
        y = m.forward_real(torch.from_numpy(data[name]).cuda())
        want = denormalize_pixel_coordinates(y)[0].cpu().numpy()
        assert want.shape == (8, 2)
        np.testing.assert_array_equal(np.asarray(got[name], np.float32), want)
