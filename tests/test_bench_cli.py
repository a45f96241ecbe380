"""bench.py's command line: a plain run computes the headline figure alone, --full adds every other
leg, --dump-outputs writes what the timed path computed in its last step."""
import numpy as np
import pytest
import torch

import bench


def test_plain_run_turns_every_other_leg_off():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert not a.full and a.steps == 7 and a.warmup == 2 and a.dump_outputs is None
    assert all(getattr(a, leg) for leg in bench.FULL_LEGS)
    f = bench.parse(["--full"])
    assert f.full and not any(getattr(f, leg) for leg in bench.FULL_LEGS)
    f = bench.parse(["--full", "--no-streaming"])
    assert f.no_streaming and not f.no_parity
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path, capsys):
    from perseus_amd import synth
    from perseus_amd.detector import KeypointCNN

    B, seed = 8, 3
    argv = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", str(B), "--seed", str(seed),
            "--dump-outputs", str(tmp_path / "out")]
    line = bench.main(argv)
    assert capsys.readouterr().out.count("\n") == 1  # the result line and nothing else
    assert (line["steps"], line["warmup"], line["dtype"], line["full"]) == (3, 1, "fp16", False)
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0
    # value and ms_per_step are the same measurement (both rounded: 0.1 frames/s, 1e-4 ms)
    assert line["value"] == pytest.approx(B / (line["ms_per_step"] * 1e-3), rel=2e-3)
    for leg in ("px_l2", "roofline", "per_kernel_roofline", "parity_mode", "fp32_mode", "trajectory_set", "streaming",
                "cpu_baseline", "factors"):
        assert line[leg] is None, leg
    assert line["kernels_ms"] == {}
    y = np.load(tmp_path / "out" / "keypoints.npy")
    assert y.dtype == np.float32 and y.shape == (B, 16)
    # the dumped array is the forward of the seeded frames through the seeded weights
    m = KeypointCNN(num_channels=4, precision="fp16")
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.synthetic_state_dict(seed).items()})
    want = m.eval()(torch.from_numpy(synth.synthetic_frames(seed, B)).cuda()).cpu().numpy()
    np.testing.assert_array_equal(y, want)
