"""Keypoints of real RGB images, the inference half of perseus/detector/validate_real.py:
the sorted `*.png` of a directory without "segmentation" in the name (:53-54), each decoded,
divided by 255, resized to a short side of int(1.8 * H) unless it is already H x W,
centre-cropped (:62-71) and run through the RGB model one image at a time
(KeypointCNN.forward_real), the keypoints denormalized to pixels of the H x W crop.  Writes
{file name: [[u, v] x K]} as JSON.  No plotting and no GIF.

    python tools/validate_real.py DIR [--weights CKPT] [--precision fp16|fp16x3|fp32] [--out FILE.json]
"""
import argparse
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def image_files(directory):
    """validate_real.py:53-54."""
    return [f for f in sorted(glob.glob(os.path.join(directory, "*.png"))) if "segmentation" not in os.path.basename(f)]


def predict(model, directory):
    """{file name: (K, 2) pixel coordinates as nested lists} over image_files(directory)."""
    import torch

    from perseus_amd.data import decode_png
    from perseus_amd.detector import denormalize_pixel_coordinates

    dev = torch.device("cuda", torch.cuda.current_device())
    out = {}
    for path in image_files(directory):
        with open(path, "rb") as fh:
            rgb = decode_png(fh.read(), rgb=True)  # PIL .convert("RGB") bytes (:62)
        y = model.forward_real(torch.from_numpy(rgb).to(dev))
        px = denormalize_pixel_coordinates(y, model.H, model.W)
        out[os.path.basename(path)] = px[0].cpu().tolist()
    return out


def load_model(weights=None, precision="fp16"):
    """The RGB KeypointCNN with a reference checkpoint (validate.py:92-98: "module." stripped),
    or synthetic weights when none is given."""
    import numpy as np
    import torch

    from perseus_amd import synth
    from perseus_amd.detector import KeypointCNN

    m = KeypointCNN(num_channels=3, precision=precision)
    if weights:
        sd = torch.load(weights, map_location="cpu", weights_only=True)
        m.load_state_dict({k.replace("module.", ""): v for k, v in sd.items()})
    else:
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.synthetic_state_dict(0, 3).items()})
    return m.eval()


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("dir")
    p.add_argument("--weights", default=None, help="state dict of the 3-channel model (default: synthetic weights)")
    p.add_argument("--precision", default="fp16", choices=("fp16", "fp16x3", "fp32"))
    p.add_argument("--out", default=None, help="JSON file (default: stdout)")
    a = p.parse_args(argv)
    res = predict(load_model(a.weights, a.precision), a.dir)
    text = json.dumps(res)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
