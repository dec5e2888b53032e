"""What the output format costs or saves: FMD_PCM_F32 against FMD_PCM_S16 (include/fmd.h) on one box, every variant
visited twice in alternation (F32, S16, F32, S16) in one process.

  device: 8192 channels x 65 536 samples, 2.4 MS/s, D = 11, a device-resident input row per channel, overlapped
          calls (concurrency 2) consumed two calls late as bench.py runs them; float and S16 *input*.  Per visit: ms
          per step; per format: MS/s of the better visit and the audio tail's own ms (a short run at profiling level
          1: the kernel's own start and stop events inside the overlapped pipeline, fmd_batch_debug_timeline).
  host:   fmd_batch_process_host_pcm, 8192 channels on one shared capture (the input copy is 512 KB, the call is
          dominated by the audio coming back): wall ms around the synchronous call, and the library's own split of it
          (fmd_batch_debug_host_ms: wait + copy out).

One JSON line, also written to profiles/pcm_formats.json.

    python tools/pcm_bench.py --steps 240 --warmup 8 [--host-calls 20] [--parts device,host]
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
from tools import fmsig_py  # noqa: E402

N, LAG, RING, C = 65536, 2, 3, 8192
FS, D = 2.4e6, 11
VISITS = ["f32", "s16", "f32", "s16"]


def make_batch(pkg):
    b = pkg.Batch(pkg.make_params(FS, -0.15 * FS, 48000.0, 15000.0, D), C, record_callbacks=False)
    b.set_concurrency(2)
    return b


def run_device(pkg, iq, in_fmt, pcm, steps, warmup, profile=False):
    b = make_batch(pkg)
    if profile:
        b.set_profiling(1)
    s16 = pcm == "s16"
    a_stride = (b.max_audio_floats(N) + 63) // 64 * 64
    audio = [torch.empty((C, a_stride), dtype=torch.int16 if s16 else torch.float32, device="cuda")
             for _ in range(LAG + 3)]
    s = torch.cuda.current_stream().cuda_stream
    t0 = None
    for j in range(warmup + steps):
        if j == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        b.process_device(iq[j % RING].data_ptr(), N, N, audio[j % len(audio)].data_ptr(), a_stride, s, fmt=in_fmt,
                         pcm=np.int16 if s16 else np.float32)
        if j >= LAG:
            b.wait(stream=s, lag=LAG)
            b.collect_rds_array(cap=4 * C, stream=s, lag=LAG)
    b.wait(stream=s)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    tail = None
    if profile:
        tl = b.debug_timeline()[warmup:]
        tail = float(np.mean(tl[:, 5] - tl[:, 4])) if len(tl) else None
    clip = int(b.pcm_clipped().sum()) if s16 else 0
    b.close()
    return ms, tail, clip


def run_host(pkg, x, pcm, calls, warmup):
    b = pkg.Batch(pkg.make_params(FS, -0.15 * FS, 48000.0, 15000.0, D), C, tuning_shifts=np.full(C, 10, np.int32),
                  record_callbacks=False)
    ms = []
    for j in range(warmup + calls):
        if j == warmup:
            b.debug_host_ms()  # restart the library's own sums
        t0 = time.perf_counter()
        b.process_host_fmt(x[j % len(x)], shared=True, pcm=np.int16 if pcm == "s16" else None)
        if j >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    _, split = b.debug_host_ms()
    b.close()
    return float(np.median(ms)), float(np.min(ms)), split


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=240)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--profile-steps", type=int, default=32)
    ap.add_argument("--host-calls", type=int, default=20)
    ap.add_argument("--parts", default="device,host")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcm_formats.json"))
    args = ap.parse_args()
    pkg = load_package()
    parts = [p for p in args.parts.split(",") if p]
    res = {"tool": "pcm_bench", "channels": C, "samples": N, "sample_rate_if": FS, "downsample": D, "lag": LAG,
           "steps": args.steps, "warmup": args.warmup, "order_of_visits": VISITS}
    if "device" in parts:
        gen = fmsig_py.DeviceGenerator([fmsig_py.channel_params(FS, c) for c in range(C)], "cuda")
        base = torch.empty((RING, C, N, 2), dtype=torch.float32, device="cuda")
        for r in range(RING):
            gen.generate(base[r], r * N, N)
        rings = {"f32": (base, pkg.FMD_IQ_F32),
                 "s16": (torch.clamp(torch.round(base * 32767.0), -32768, 32767).to(torch.int16).contiguous(),
                         pkg.FMD_IQ_S16)}
        torch.cuda.synchronize()
        res["device"] = {}
        for in_name, (iq, in_fmt) in rings.items():
            visits = {"f32": [], "s16": []}
            for pcm in VISITS:
                visits[pcm].append(round(run_device(pkg, iq, in_fmt, pcm, args.steps, args.warmup)[0], 4))
            out = {}
            for pcm in ("f32", "s16"):
                _, tail, clip = run_device(pkg, iq, in_fmt, pcm, args.profile_steps, args.warmup, profile=True)
                out[pcm] = {"ms_per_step": visits[pcm],
                            "ms_samples_per_s": round(C * N / (min(visits[pcm]) * 1e-3) / 1e6, 1),
                            "audio_tail_ms": None if tail is None else round(tail, 4),
                            "audio_bytes_per_call": C * b_audio_samples(pkg) * pkg.PCM_BYTES[1 if pcm == "s16" else 0],
                            "samples_clipped_in_profile_run": clip}
            out["s16_best_vs_f32_slower_visit"] = round(max(visits["f32"]) / min(visits["s16"]) - 1.0, 4)
            out["s16_no_slower_than_slower_f32_visit"] = min(visits["s16"]) <= max(visits["f32"])
            res["device"]["input_" + in_name] = out
        del base, rings
        torch.cuda.empty_cache()
    if "host" in parts:
        p = fmsig_py.default_params(FS, noise_sigma=0.005)
        x = [fmsig_py.generate_f32(p, r * N, N) for r in range(RING)]
        visits = {"f32": [], "s16": []}
        for pcm in VISITS:
            med, best, split = run_host(pkg, x, pcm, args.host_calls, 3)
            visits[pcm].append({"wall_ms_median": round(med, 3), "wall_ms_min": round(best, 3),
                                "library_ms": {k: round(v, 3) for k, v in split.items()}})
        res["host"] = {"calls_per_visit": args.host_calls, "input": "one shared capture, float", "visits": visits,
                       "s16_over_f32_wall": round(min(v["wall_ms_median"] for v in visits["s16"]) /
                                                  min(v["wall_ms_median"] for v in visits["f32"]), 4)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


def b_audio_samples(pkg):
    """audio samples per channel of one full call at this geometry (both formats: a sample count)"""
    b = pkg.Batch(pkg.make_params(FS, -0.15 * FS, 48000.0, 15000.0, D), 1, record_callbacks=False)
    n = b.max_audio_floats(N)
    b.close()
    return n


if __name__ == "__main__":
    main()
