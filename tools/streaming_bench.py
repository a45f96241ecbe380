"""Config 4: 3 x 720p RGBD cameras at 30 Hz, end-to-end keypoint and pose latency on 1 GPU.

The measurement is bench.py's `streaming_leg` (the same numbers appear in every
`bench.py --full` line as "streaming"): per tick, stage the 3 frames (host -> pinned, centre crop), one
hipGraph replay (H2D, preprocess, B=3 forward, denormalize, D2H; with the pose stage
also window advance, factor linearize, GN step, retract, D2H poses), wait.  Prints one
JSON line.

    python tools/streaming_bench.py [--ticks 300] [--hz 30] [--window 24] [--channels {3,4}] [--timed 1]
                                      [--gate CHI2]

--gate CHI2 (only with --timed 1; default off) switches the keypoint gate on (StreamingPipeline(
gate_chi2=CHI2): the window's marginals, pa_window_predict and pa_keypoint_gate inside the tick's
graph), so the tick latency can be read with and without it; the report gains "gate_chi2" and the
number of cameras whose gate applied on the last tick.

--timed 1 runs the pose tick with real timestamps (StreamingPipeline(timed=True)): seeded +-30 %
stamp jitter per camera, the same report fields for the one mode "pose".

--channels 3 runs the same ticks with the RGB model (the colour frames alone are staged; the
fp16 modes only).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_leg(model, dev, ticks, hz, cams, window, zero_copy, zero_copy_out, seed=0, jitter=0.3, gate=None):
    """bench.streaming_leg's "pose" mode with StreamingPipeline(timed=True): every tick is given
    per-camera stamps with seeded +-`jitter` period jitter (the pacing itself stays at `hz`), so
    the tick stages and copies its [dt_new | mask_new] block.  The same report fields.
    The frames, the pacing loop, the percentiles and the 20-replay device timing are copied from
    bench.streaming_leg (bench.py is the fixed yardstick and has no hook for per-tick keywords):
    a change to the measurement there has to be repeated here."""
    import time

    import numpy as np
    import torch

    from perseus_amd.streaming import StreamingPipeline

    rng = np.random.default_rng(0)
    n_src = 8
    rgbs = rng.integers(0, 256, (n_src, cams, 720, 1280, 3), dtype=np.uint8)
    deps = rng.uniform(0.12, 0.48, (n_src, cams, 720, 1280)).astype(np.float32)
    pipe = StreamingPipeline(model, n_cams=cams, graph=True, host_crop=True, device=dev, zero_copy=zero_copy,
                             zero_copy_out=zero_copy_out, pose_window=window, proj_sigma=40.0, timed=True,
                             gate_chi2=gate)
    jr = np.random.default_rng(seed)
    period = 1.0 / hz
    stamps = np.zeros(cams)

    def tick(i):
        nonlocal stamps
        stamps = stamps + period * (1.0 + jitter * jr.uniform(-1.0, 1.0, cams))
        pipe.tick(rgbs[i % n_src], deps[i % n_src], stamps=stamps)

    for i in range(10):
        tick(i)
    lat = []
    t_next = time.perf_counter()
    for i in range(ticks):
        while time.perf_counter() < t_next:
            pass
        t0 = time.perf_counter()
        tick(i)
        lat.append(time.perf_counter() - t0)
        t_next += period
    lat = np.array(lat) * 1e3
    s = pipe.stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        e0.record(s)
        for _ in range(20):
            pipe.replay()
        e1.record(s)
    s.synchronize()
    r = {"ticks": ticks, "p50_ms": round(float(np.percentile(lat, 50)), 4),
         "p99_ms": round(float(np.percentile(lat, 99)), 4), "max_ms": round(float(lat.max()), 4),
         "device_ms_per_tick": round(e0.elapsed_time(e1) / 20, 4), "window_frames": window,
         "precision": pipe.model.precision, "timed": True, "stamp_jitter": jitter,
         "solved_last_tick": int((pipe.info_h.numpy() == 0).sum())}
    if gate is not None:
        r.update(gate_chi2=gate, gate_applied_last_tick=int((pipe.gate_state()["ginfo"] == 0).sum()))
    pipe.close()
    return {"workload": f"configs[4]: {cams} x 720p RGBD @ {hz:g} Hz, centre crop 256, B = {cams} per tick, timed",
            "unit": "ms", "timing": "host time from staging start to results on the host, paced ticks", "pose": r}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--ticks", type=int, default=300)
    p.add_argument("--hz", type=float, default=30.0)
    p.add_argument("--cams", type=int, default=3)
    p.add_argument("--window", type=int, default=24)
    p.add_argument("--zero-copy", type=int, default=None, help="1 / 0: the tick reads the pinned staging (no H2D copy); default per precision")
    p.add_argument("--zero-copy-out", type=int, default=1, help="1 / 0: results written into the pinned block (no D2H copy)")
    p.add_argument("--channels", type=int, default=4, choices=(3, 4),
                   help="3: the RGB model (the tick stages and reads the colour frames alone; fp16 modes only)")
    p.add_argument("--timed", type=int, default=0,
                   help="1: the pose tick with real timestamps (StreamingPipeline(timed=True)), seeded +-30 %% stamp jitter")
    p.add_argument("--gate", type=float, default=None, metavar="CHI2",
                   help="the keypoint gate's chi-square bound (e.g. 13.816); needs --timed 1; default: no gate")
    a = p.parse_args()
    if a.gate is not None and not a.timed:
        p.error("--gate needs --timed 1 (the gate writes the keypoint masks)")
    import numpy as np
    import torch

    from bench import streaming_leg
    from perseus_amd import synth
    from perseus_amd.detector import KeypointCNN

    m = KeypointCNN(num_channels=a.channels)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v))
                       for k, v in synth.synthetic_state_dict(0, a.channels).items()})
    dev = torch.device("cuda", 0)
    if a.timed:
        print(json.dumps(timed_leg(m, dev, a.ticks, a.hz, a.cams, a.window,
                                   None if a.zero_copy is None else bool(a.zero_copy), bool(a.zero_copy_out),
                                   gate=a.gate)))
        return
    kw = {}
    if a.channels == 3:  # (the leg's parity modes build their own 4-channel fp16x3 model)
        kw["modes"] = ("pose", "pose_ahead", "pixels")
    res = streaming_leg(m, dev, a.ticks, a.hz, a.cams, a.window, zero_copy=None if a.zero_copy is None else bool(a.zero_copy),
                        zero_copy_out=bool(a.zero_copy_out), **kw)
    if a.channels == 3:  # the leg's own labels speak of RGBD
        res["workload"] = res["workload"].replace("RGBD", "RGB (3-channel model, depth ignored)")
        for r in res.values():
            if isinstance(r, dict) and "stage" in r:
                r["stage"] = r["stage"].replace("forward_rgbd_px", "forward_rgb_px")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
