"""Cost of capture maps and capture switches (fmd_batch_set_capture_map / fmd_batch_switch_captures) at the headline
geometry: 32 captures x 256 stations = 8192 channels x 65 536 samples, 2.4 MS/s, D = 11, overlapped calls consumed
two calls late, as bench.py runs them.  Prints one JSON line per part.

  layouts:  ms per step (and the IF FIR's own ms from a profiled run of its own) with channels_per_capture = 256,
            the same assignment as an explicit map, a shuffled map with the capture-ordered walk and without it
  switches: ms per step with R channels switched to other captures in front of every call (shuffled map)

    python tools/capture_switch_bench.py --steps 240 --warmup 8 [--part layouts|switches|both]
    python tools/capture_switch_bench.py --steps 16 --only shuffled_walk     (one layout, e.g. under a counter run)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

N, FS, D, LAG, G, K = 65536, 2.4e6, 11, 2, 32, 256
LAYOUTS = ["channels_per_capture", "explicit_map", "shuffled_walk", "shuffled_no_walk"]


def make_batch(pkg, layout):
    C = G * K
    rng = np.random.default_rng(3)
    shifts = rng.integers(-24, 24, size=C).astype(np.int32)
    b = pkg.Batch(pkg.make_params(FS, 0.0, 48000.0, 15000.0, D), C, tuning_shifts=shifts, record_callbacks=False)
    cmap = np.arange(C, dtype=np.uint32) // K
    if layout == "channels_per_capture":
        b.set_channels_per_capture(K)
    elif layout == "explicit_map":
        b.set_capture_map(cmap, G)
    else:
        b.set_capture_map(cmap[rng.permutation(C)], G)
        b.debug_capture_walk(1 if layout == "shuffled_walk" else 0)
    b.set_concurrency(2)
    return b


def run(pkg, layout, steps, warmup, R=0, profile=False):
    b = make_batch(pkg, layout)
    C = G * K
    if profile:
        b.set_profiling(1)
    torch.manual_seed(1)
    iq = (0.1 * torch.randn((G, N, 2), dtype=torch.float32, device="cuda")).contiguous()
    a_stride = (b.max_audio_floats(N) + 63) // 64 * 64
    audio = [torch.empty((C, a_stride), dtype=torch.float32, device="cuda") for _ in range(LAG + 2)]
    s = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(7)
    t0 = None
    for j in range(warmup + steps):
        if j == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        if R:
            ch = rng.choice(C, size=R, replace=False).astype(np.uint32)
            b.switch_captures(ch, rng.integers(0, G, size=R).astype(np.uint32))
        b.process_device(iq.data_ptr(), N, N, audio[j % len(audio)].data_ptr(), a_stride, s)
        if j >= LAG:
            b.wait(stream=s, lag=LAG)
        if j % 8 == 7:
            b.collect_rds(lag=LAG)
    b.wait(stream=s)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    fir = b.stage_ms()[0]["if_fir"] if profile else None
    b.close()
    return ms, fir


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=240)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--part", default="both", choices=["layouts", "switches", "both"])
    ap.add_argument("--only", default=None, choices=LAYOUTS, help="one layout, no profiled run")
    ap.add_argument("--switches", default="0,1,64,8192")
    ap.add_argument("--repeats", type=int, default=2, help="alternated runs of every variant")
    args = ap.parse_args()
    pkg = load_package()
    if args.only:
        ms, _ = run(pkg, args.only, args.steps, args.warmup)
        print(json.dumps({"part": "layout", "layout": args.only, "ms_per_step": ms, "steps": args.steps}))
        return
    if args.part in ("layouts", "both"):
        res = {"part": "layouts", "channels": G * K, "captures": G, "samples": N, "steps": args.steps}
        for rep in range(args.repeats):  # alternated: every layout once per round
            for lay in LAYOUTS:
                ms, _ = run(pkg, lay, args.steps, args.warmup)
                res.setdefault(lay + "_ms_per_step", []).append(round(ms, 4))
        for lay in LAYOUTS:
            _, fir = run(pkg, lay, min(args.steps, 64), args.warmup, profile=True)
            res[lay + "_if_fir_ms"] = round(fir, 4)
        base = min(res["channels_per_capture_ms_per_step"])
        for lay in LAYOUTS[1:]:
            res[lay + "_vs_channels_per_capture"] = round(min(res[lay + "_ms_per_step"]) / base - 1.0, 4)
        res["ms_samples_per_s"] = round(G * K * N / (base * 1e-3) / 1e6, 1)
        print(json.dumps(res))
    if args.part in ("switches", "both"):
        res = {"part": "switches", "channels": G * K, "captures": G, "samples": N, "steps": args.steps,
               "layout": "shuffled_walk", "lag": LAG}
        rs = [int(x) for x in args.switches.split(",") if x != ""]
        for rep in range(args.repeats):
            for r in rs:
                ms, _ = run(pkg, "shuffled_walk", args.steps, args.warmup, R=r)
                res.setdefault("R%d_ms_per_step" % r, []).append(round(ms, 4))
        base = min(res["R0_ms_per_step"])
        for r in rs[1:]:
            res["R%d_us_per_call_over_R0" % r] = round((min(res["R%d_ms_per_step" % r]) - base) * 1e3, 1)
        print(json.dumps(res))


if __name__ == "__main__":
    main()
